"""Comparing two calibrations in pixel space on the device (vc_compar*, vicalib_amd/csrc/vc_compare.hip): the kernels against the numpy reference
and the checks of tests/compare_cases.py (the ones tests/test_compare_cpu.py applies to the host build of the same arithmetic), their
determinism, the smallest lattice, a full 640 x 480 lattice of 1200 workgroups, a calibrator's camera, and the command line."""
import os
import subprocess

import numpy as np
import pytest

import compare_cases as cc
import rectify_cases as rc
import undistort_cases as uc
import vicalib_amd.lib as lib
from vicalib_amd import synth
from vicalib_amd.lib import Comparer, ViCalibrator

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")


def comparer(c, size=cc.SIZE, grid=cc.GRID):
    return Comparer(c.cams[0], c.cams[1], size, grid)


def collect(cmp, ring_counts=cc.RING_COUNTS):
    """the last run of a Comparer in the layout the checks take"""
    out = cmp.fit()
    d, f = cmp.map()
    out.update(diff=d.reshape(-1, 2), flags=f.reshape(-1), summary=cmp.summary(), rings={n: cmp.rings(n) for n in ring_counts})
    return out


def same_bits(a, b):
    flat = lambda o: [o[k] for k in ("R", "status", "iterations", "n_fit", "n_left_out", "cost0", "cost", "diff", "flags")] + \
        [o["summary"][k] for k in sorted(o["summary"])] + [r[k] for _, r in sorted(o["rings"].items()) for k in sorted(r)]      # noqa: E731
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(flat(a), flat(b)))


@pytest.mark.parametrize("name", cc.case_names())
def test_cases_against_numpy(name):
    """checks 1 - 6, then the same bits from a second run of the handle and from a second handle"""
    cmp = comparer(cc.case(name))

    def run(c, fit_radius, R_ba):
        cmp.run(fit_radius, 0, R_ba)
        return collect(cmp)
    first = cc.check_case(name, run)
    again = run(None, cc.case(name).fit_radius, None)
    other = comparer(cc.case(name))
    other.run(cc.case(name).fit_radius)
    assert same_bits(first, again) and same_bits(first, collect(other))


def test_readers_before_a_run_and_given_rotation():
    c = cc.case("shift")
    cmp = comparer(c)
    for read in (cmp.fit, cmp.map, cmp.summary, cmp.rings, cmp.time):
        with pytest.raises(lib.VicalibError, match="BAD_ARG"):
            read()
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        cmp.run(0.0, 0, 1.001 * np.eye(3))                       # not a rotation
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        cmp.summary()                                            # a refused run leaves nothing to read
    R = cc.rot([0.004, -0.002, 0.01])
    out = cmp.run(0.0, 0, R)
    assert np.array_equal(out["R"], R) and out["iterations"] == 0
    ref = cc.reference("shift")
    d_ref, valid = ref.diff(R)
    d, f = cmp.map()
    assert valid.all() and not f.any() and np.abs(d.reshape(-1, 2) - d_ref).max() <= 1e-8
    cc.check_sums(ref.rho, collect(cmp))
    # the fit does not read R_ba, and an iteration cap of one step ends with status 1
    capped = cmp.run(0.5, 1, 1.001 * np.eye(3))
    assert capped["status"] == 1 and capped["iterations"] == 1 and capped["cost"] < capped["cost0"]
    assert (cmp.time(2) > 0).all()


def test_smallest_lattice():
    """2 x 2: the four corners, rho = 1.  With fit_radius = 1.5 they are the fit set and the fit runs; with 0.5 the set is empty"""
    c = cc.case("shift")
    cmp = comparer(c, grid=(2, 2))
    out = cmp.run(1.5)
    assert out["n_fit"] == 4 and out["n_left_out"] == 0 and out["status"] in (0, 1, 2) and out["cost"] <= out["cost0"]
    q, rho = cc.lattice(cc.SIZE, (2, 2))
    assert np.array_equal(rho, np.ones(4))
    res = collect(cmp)
    cc.check_sums(rho, res)
    assert res["summary"]["count"] == 4 and res["rings"][8]["count"][7] == 4
    with pytest.raises(lib.VicalibError, match="NUMERIC"):
        cmp.run(0.5)
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        cmp.summary()


def test_full_lattice():
    """640 x 480 samples, 1200 workgroups, the rings in LDS: check 6, the same bits twice, and consistency with the 53 x 41 run of the case"""
    c = cc.case("shift")
    full, small = comparer(c, grid=cc.SIZE), comparer(c)
    a = full.run(0.5); first = collect(full)
    full.run(0.5); again = collect(full)
    assert same_bits(first, again)
    q, rho = cc.lattice(cc.SIZE, cc.SIZE)
    cc.assert_thresholds_decided(rho, 0.5)
    cc.check_sums(rho, first)
    b = small.run(0.5)
    s_full, s_small = full.summary(), small.summary()
    assert s_full["count"] == 640 * 480 and s_full["invalid"] == 0
    rms_full, rms_small = np.sqrt(s_full["sum_sq"] / s_full["count"]), np.sqrt(s_small["sum_sq"] / s_small["count"])
    between = cc.angle(a["R"] @ b["R"].T)
    print("shift: compensated rms %.4f px on 640 x 480, %.4f px on 53 x 41; implied rotations %.3g rad apart" % (rms_full, rms_small, between))
    assert rms_small / 1.5 <= rms_full <= 1.5 * rms_small
    assert between <= 1e-4


@pytest.mark.parametrize("grid,fit_radius", cc.BOUNDARY_LATTICES)
def test_workgroup_boundary_lattices(grid, fit_radius):
    """the shift case where a sweep or a fit fills its workgroups exactly or by one or two samples more, rings at 1, 5, 8 and 64: check 6 and
    the same bits from a second run"""
    q, rho = cc.lattice(cc.SIZE, grid)
    cc.assert_thresholds_decided(rho, 0.5, cc.BOUNDARY_RING_COUNTS)
    cc.assert_thresholds_decided(rho, fit_radius, cc.BOUNDARY_RING_COUNTS)
    cmp = comparer(cc.case("shift"), grid=grid)
    fit = cmp.run(fit_radius)
    first = collect(cmp, cc.BOUNDARY_RING_COUNTS)
    assert fit["n_fit"] == (rho <= fit_radius).sum() and fit["n_left_out"] == 0 and first["summary"]["count"] == grid[0] * grid[1]
    cc.check_sums(rho, first)
    cmp.run(fit_radius)
    assert same_bits(first, collect(cmp, cc.BOUNDARY_RING_COUNTS))


def test_for_camera_of_a_calibrator():
    """a calibrator that only had a camera added: A is that camera"""
    c = cc.case("cross")
    (ma, Ka), (mb, Kb) = c.cams
    cal = ViCalibrator(0)
    cal.AddCamera(synth.MODEL_IDS[ma], Ka, rc.IDENTITY_POSE, cc.SIZE[0], cc.SIZE[1])
    mine = Comparer.for_camera(cal, 0, (mb, Kb), cc.GRID)
    mine.run(0.5)
    plain = comparer(c)
    plain.run(0.5)
    assert same_bits(collect(mine), collect(plain))
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        Comparer.for_camera(cal, 1, (mb, Kb), cc.GRID)


# ---------------------------------------------------------------------------------------------------------------- the command line
def _csv(path, header):
    lines = open(path).read().splitlines()
    assert lines[0] == header, lines[0]
    return lines[1:]


def _written_rig(cams, path, calibrate_imu):
    """a rig file from the calibrator's own writer (robotics axes with calibrate_imu)"""
    cal = ViCalibrator(0)
    for m, K, T in cams:
        cal.AddCamera(m, K, T, cc.SIZE[0], cc.SIZE[1])
    cal.SetCalibrateImu(calibrate_imu)
    cal.WriteCameraModels(str(path))


def test_cli_compare_models(tmp_path):
    """two rig files of two cameras from vc_write_camera_models, one with the robotics axes; camera 0's principal point and camera 1's pose
    moved in the second: the CSVs hold the Comparer's arrays, and the poses come back from the files to 1e-12"""
    Ta0, Ta1 = rc.hand_rig()
    (R1, t1) = rc.pose_Rt(Ta1)
    Tb1 = rc.pose(cc.rot([0.002, -0.004, 0.001]) @ R1, t1 + [0.001, 0.0, -0.002])
    K3, K4 = uc.gt("poly3"), uc.gt("kb4")
    K3b = K3 + np.array([0, 0, 3.0, -2.0, 0, 0, 0])
    a, b, out = tmp_path / "a.xml", tmp_path / "b.xml", tmp_path / "cmp"
    _written_rig([("poly3", K3, Ta0), ("kb4", K4, Ta1)], a, False)
    _written_rig([("poly3", K3b, Ta0), ("kb4", K4, Tb1)], b, True)
    r = subprocess.run([BIN, "-compare_models", "%s,%s" % (a, b), "-compare_dir", str(out), "-compare_grid", "%dx%d" % cc.GRID, "-compare_rings", "5"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    q, rho = cc.lattice()
    implied, summary_rows = [], _csv(out / "compare_summary.csv", "camera,model_a,model_b,rx_deg,ry_deg,rz_deg,status,iterations,n_fit,count,invalid,rms_px,max_px,"
                                                                  "count_plain,rms_plain_px,max_plain_px")
    assert summary_rows[2] == "camera,ring,rho_from,rho_to,count,invalid,rms_px,max_px" and len(summary_rows) == 3 + 2 * 5
    for cam, (A, B) in enumerate(((("poly3", K3), ("poly3", K3b)), (("kb4", K4), ("kb4", K4)))):
        cmp = Comparer(A, B, cc.SIZE, cc.GRID)
        fit = cmp.run(0.5)
        d, f = cmp.map()
        rows = np.array([[float(x) for x in line.split(",")] for line in _csv(out / ("compare_cam%d.csv" % cam), "x,y,du,dv,flags")])
        assert np.array_equal(rows[:, :2], q) and np.array_equal(rows[:, 2:4], d.reshape(-1, 2), equal_nan=True) and np.array_equal(rows[:, 4], f.reshape(-1))
        s, rings = cmp.summary(), cmp.rings(5)
        row = summary_rows[cam].split(",")
        assert row[:3] == [str(cam), A[0], B[0]] and int(row[6]) == fit["status"] and int(row[8]) == fit["n_fit"] and int(row[9]) == s["count"]
        from scipy.spatial.transform import Rotation
        assert np.abs(np.array(row[3:6], dtype=float) - np.degrees(Rotation.from_matrix(fit["R"]).as_rotvec())).max() <= 1e-9
        assert float(row[11]) == np.sqrt(s["sum_sq"] / s["count"]) and float(row[12]) == s["max_err"]
        for k in range(5):
            ring = summary_rows[3 + 5 * cam + k].split(",")
            assert [int(ring[0]), int(ring[1]), int(ring[4])] == [cam, k, rings["count"][k]] and float(ring[7]) == rings["max_err"][k]
        plain = cmp.run(0.0)
        sp = cmp.summary()
        assert float(row[14]) == np.sqrt(sp["sum_sq"] / sp["count"]) and plain["iterations"] == 0
        implied.append(fit["R"])
    assert abs(float(summary_rows[0].split(",")[14]) - np.sqrt(13.0)) <= 1e-8 and float(summary_rows[1].split(",")[14]) <= 1e-8
    ext = [np.array(line.split(","), dtype=float) for line in _csv(out / "compare_extrinsics.csv", "camera,angle_deg,distance_m,angle_plain_deg,distance_plain_m,"
           "a_qx,a_qy,a_qz,a_qw,a_tx,a_ty,a_tz,b_qx,b_qy,b_qz,b_qw,b_tx,b_ty,b_tz")]
    assert len(ext) == 2
    for row, Ta, Tb in zip(ext, (Ta0, Ta1), (Ta0, Tb1)):
        for got, want in ((row[5:12], Ta), (row[12:19], Tb)):
            got = got * np.sign(got[3] * want[3])                     # (q and -q are the same rotation)
            assert np.abs(got - want).max() <= 1e-12
    want = Comparer.extrinsics(Ta0, Ta1, Ta0, Tb1, implied[0], implied[1])
    got = ext[1][1:5] * [np.pi / 180, 1, np.pi / 180, 1]
    print("camera 1 against 0: compensated %.3g rad %.3g m, plain %.3g rad %.3g m" % tuple(got))
    assert np.abs(got - want).max() <= 1e-12 and np.abs(ext[0][1:5]).max() <= 1e-12
    assert got[2] > 1e-3 and got[3] > 1e-3


def test_cli_compare_to(tmp_path):
    """a small vision-only solve compared with the ground truth it was generated from: the files hold what a Comparer gives for the camera the
    tool wrote into cameras.xml (its parameters are printed with 17 digits) against the file's"""
    import re
    prob = synth.generate(synth.Config(models=("poly3",), n_frames=12, seed=3))
    files, _ = synth.write_dataset(prob, str(tmp_path))
    truth, result = tmp_path / "truth.xml", tmp_path / "cameras.xml"
    size = (prob.cfg.width, prob.cfg.height)
    truth.write_text(cc.rig_xml([("poly3", prob.cam_K_gt[0], prob.cam_T_ck_gt[0])], size=size))
    out = tmp_path / "cmp"
    r = subprocess.run([BIN, "-cam", "detections://" + ",".join(files), "-models", "poly3", "-nocalibrate_imu", "-output", str(result),
                        "-compare_to", str(truth), "-compare_dir", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    K = np.array([float(x) for x in re.search(r"<params> \[(.*?)\] </params>", result.read_text()).group(1).split(";")])
    assert len(K) == 7
    cmp = Comparer(("poly3", K), ("poly3", prob.cam_K_gt[0]), size)
    fit = cmp.run(0.5)
    d, f = cmp.map()
    s = cmp.summary()
    rows = _csv(out / "compare_summary.csv", "camera,model_a,model_b,rx_deg,ry_deg,rz_deg,status,iterations,n_fit,count,invalid,rms_px,max_px,count_plain,rms_plain_px,max_plain_px")
    row = rows[0].split(",")
    print("solve against ground truth: %s px rms compensated (%s px max), %s px plain" % (row[11], row[12], row[14]))
    assert len(rows) == 2 + 8 and row[1:3] == ["poly3", "poly3"] and int(row[6]) == fit["status"] and int(row[9]) == s["count"] == 64 * 48
    assert float(row[11]) == np.sqrt(s["sum_sq"] / s["count"]) and float(row[12]) == s["max_err"]
    got = np.array([[float(x) for x in line.split(",")] for line in _csv(out / "compare_cam0.csv", "x,y,du,dv,flags")])
    assert np.array_equal(got[:, 2:4], d.reshape(-1, 2), equal_nan=True) and np.array_equal(got[:, 4], f.reshape(-1))
    assert not (out / "compare_extrinsics.csv").exists()
