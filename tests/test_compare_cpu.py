"""Comparing two calibrations in pixel space (vc_compar*), the part that needs no GPU: the comparison's arithmetic (vc_compare.hpp) compiled
for the host and held to the same numpy reference and the same checks that tests/test_compare_gpu.py applies to the kernels, the extrinsics
(host entry point of the library), argument errors, the refusal to run without a device, and the command line's flag and rig-file errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import compare_cases as cc
import rectify_cases as rc
import undistort_cases as uc
import vicalib_amd.lib as lib
from vicalib_amd import synth
from vicalib_amd.lib import Comparer

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _harness():
    src = os.path.join(HERE, "host_harness", "compare_harness.cpp")
    so = os.path.join(HERE, "host_harness", "libvc_compare_harness.so")
    deps = [src] + [os.path.join(ROOT, "vicalib_amd", "csrc", f) for f in ("vc_compare.hpp", "vc_rectify.hpp", "vc_undistort.hpp", "vc_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_run(c, fit_radius, R_ba, size=cc.SIZE, grid=cc.GRID, max_iters=0, ring_counts=cc.RING_COUNTS):
    """the host build of a whole run, in the layout the checks take; (status, dict)"""
    (ma, Ka), (mb, Kb) = c.cams
    n = grid[0] * grid[1]
    out = None
    rings = {}
    for nr in ring_counts:
        fit = np.zeros(15); diff = np.zeros((n, 2)); flags = np.zeros(n, dtype=np.uint8); summ = np.zeros(7); rg = np.zeros((nr, 4))
        Ka, Kb = np.ascontiguousarray(Ka, dtype=np.float64), np.ascontiguousarray(Kb, dtype=np.float64)
        st = _harness().vch_run(synth.MODEL_IDS[ma], _p(Ka), len(Ka), synth.MODEL_IDS[mb], _p(Kb), len(Kb), size[0], size[1], grid[0], grid[1],
                                C.c_double(fit_radius), int(max_iters), None if R_ba is None else _p(np.ascontiguousarray(R_ba, dtype=np.float64)), nr,
                                _p(fit), _p(diff), _p(flags), _p(summ), _p(rg))
        if st != 0:
            return st, None
        rings[nr] = dict(count=rg[:, 0].astype(np.int64), invalid=rg[:, 1].astype(np.int64), sum_sq=rg[:, 2].copy(), max_err=rg[:, 3].copy())
        if out is None:
            out = dict(R=fit[:9].reshape(3, 3).copy(), status=int(fit[9]), iterations=int(fit[10]), n_fit=int(fit[11]), n_left_out=int(fit[12]), cost0=fit[13],
                       cost=fit[14], diff=diff, flags=flags,
                       summary=dict(count=int(summ[0]), invalid=int(summ[1]), sum_du=summ[2], sum_dv=summ[3], sum_sq=summ[4], max_err=summ[5], worst=int(summ[6])))
    out["rings"] = rings
    return 0, out


# ---------------------------------------------------------------------------------------------------------------- checks 1 - 6 on the host build
@pytest.mark.parametrize("name", cc.case_names())
def test_host_arithmetic(name):
    def run(c, fit_radius, R_ba):
        st, out = host_run(c, fit_radius, R_ba)
        assert st == 0
        return out
    cc.check_case(name, run)


def test_shift_numbers():
    """what the shift case looks like: 3.606 px at R = I, a rotation of about half a degree absorbs all but a tenth of it inside the fit set"""
    ref = cc.reference("shift")
    _, plain = host_run(ref.c, 0.0, None, ring_counts=(8,))
    _, fitted = host_run(ref.c, 0.5, None, ring_counts=(8,))
    assert abs(np.sqrt(plain["summary"]["sum_sq"] / plain["summary"]["count"]) - np.sqrt(13.0)) <= 1e-8
    assert 0.4 < np.degrees(cc.angle(fitted["R"])) < 0.65
    assert fitted["status"] == 0 and 1 <= fitted["iterations"] <= 8
    assert fitted["summary"]["sum_sq"] < 0.05 * plain["summary"]["sum_sq"]


def test_given_rotation_and_small_lattices():
    ref = cc.reference("shift")
    R = cc.rot([0.004, -0.002, 0.01])
    st, out = host_run(ref.c, 0.0, R, ring_counts=(8,))
    assert st == 0 and np.array_equal(out["R"], R)
    d_ref, valid = ref.diff(R)
    assert valid.all() and np.abs(out["diff"] - d_ref).max() <= 1e-8
    assert host_run(ref.c, 0.0, 1.001 * R, ring_counts=(8,))[0] == -2          # not a rotation
    # 2 x 2: the four corners, at rho = 1
    st, out = host_run(ref.c, 1.5, None, grid=(2, 2), ring_counts=(8,))
    assert st == 0 and out["n_fit"] == 4 and out["rings"][8]["count"][7] == 4
    assert host_run(ref.c, 0.5, None, grid=(2, 2), ring_counts=(8,))[0] == -6      # nothing in the fit set: VC_ERR_NUMERIC


# ---------------------------------------------------------------------------------------------------------------- extrinsics
def _numpy_extrinsics(Ta0, Tac, Tb0, Tbc, R0, Rc):
    Ra, _, ca = rc.relative(Ta0, Tac); Rb, _, cb = rc.relative(Tb0, Tbc)
    return cc.angle(Rb.T @ Rc @ Ra @ R0.T), np.linalg.norm(cb - R0 @ ca)


def test_extrinsics_against_numpy():
    Ta0, Tac = rc.hand_rig()
    Tb0, Tbc = rc.hand_rig(True)
    R0, Rc = cc.rot([0.01, -0.02, 0.005]), cc.rot([-0.004, 0.003, 0.02])
    got = Comparer.extrinsics(Ta0, Tac, Tb0, Tbc, R0, Rc)
    want = _numpy_extrinsics(Ta0, Tac, Tb0, Tbc, R0, Rc) + _numpy_extrinsics(Ta0, Tac, Tb0, Tbc, np.eye(3), np.eye(3))
    assert np.abs(got - want).max() <= 1e-12
    assert np.array_equal(Comparer.extrinsics(Ta0, Tac, Tb0, Tbc)[:2], got[2:])           # NULL rotations are identities


def test_extrinsics_of_a_rig_consistent_under_its_implied_rotations():
    """rig B is rig A with camera 0's rays turned by R0 and camera c's by Rc: compensated, nothing is left; plain, the change shows"""
    Ta0, Tac = rc.hand_rig()
    R0, Rc = cc.rot([0.02, -0.01, 0.015]), cc.rot([-0.01, 0.025, 0.005])
    (Ra0, ta0), (Rac, tac) = rc.pose_Rt(Ta0), rc.pose_Rt(Tac)
    Tb0, Tbc = rc.pose(R0 @ Ra0, R0 @ ta0), rc.pose(Rc @ Rac, Rc @ tac)
    out = Comparer.extrinsics(Ta0, Tac, Tb0, Tbc, R0, Rc)
    print("compensated %.3g rad %.3g m, plain %.3g rad %.3g m" % tuple(out))
    assert out[0] <= 1e-12 and out[1] <= 1e-12
    assert out[2] > 0.01 and out[3] > 1e-3


def test_extrinsics_argument_errors():
    L = lib.load()
    Ta0, Tac = rc.hand_rig()
    out = np.zeros(4)
    bad = Ta0.copy(); bad[3] += 0.1
    assert L.vc_compare_extrinsics(_p(bad), _p(Tac), _p(Ta0), _p(Tac), None, None, _p(out)) == -2
    assert L.vc_compare_extrinsics(_p(Ta0), _p(Tac), _p(Ta0), _p(Tac), _p(1.01 * np.eye(3)), None, _p(out)) == -2
    assert L.vc_compare_extrinsics(_p(Ta0), _p(Tac), _p(Ta0), None, None, None, _p(out)) == -2
    assert L.vc_compare_extrinsics(_p(Ta0), _p(Tac), _p(Ta0), _p(Tac), None, None, _p(out)) == 0 and np.abs(out).max() <= 1e-15


# ---------------------------------------------------------------------------------------------------------------- the handle without a device
def _create(ma, Ka, mb, Kb, size, grid):
    h = C.c_void_p()
    Ka, Kb = np.ascontiguousarray(Ka, dtype=np.float64), np.ascontiguousarray(Kb, dtype=np.float64)
    st = lib.load().vc_comparer_create(0, synth.MODEL_IDS[ma], _p(Ka), len(Ka), synth.MODEL_IDS[mb], _p(Kb), len(Kb), size[0], size[1], grid[0], grid[1], C.byref(h))
    if h.value:
        lib.load().vc_comparer_destroy(h)
    return st


def test_argument_errors_come_before_the_device():
    K3, K4 = uc.gt("poly3"), uc.gt("kb4")
    assert _create("poly3", K3, "kb4", K4, (640, 480), (641, 48)) == -2          # a grid above the image
    assert _create("poly3", K3, "kb4", K4, (640, 480), (64, 481)) == -2
    assert _create("poly3", K3, "kb4", K4, (640, 480), (1, 48)) == -2
    assert _create("poly3", K3, "kb4", K4, (4096, 4096), (2049, 2048)) == -2     # above 2^22 samples
    assert _create("poly3", K3[:6], "kb4", K4, (640, 480), (64, 48)) == -2       # a wrong nparams
    assert _create("poly3", K3, "kb4", K4[:7], (640, 480), (64, 48)) == -2
    assert _create("poly3", K3, "kb4", K4, (640, 1), (64, 2)) == -2
    L = lib.load()
    assert L.vc_compare_run(None, C.c_double(0.5), 0, None) == -2
    assert L.vc_compare_get_fit(None, None, None, None, None, None, None, None) == -2
    assert L.vc_compare_get_map(None, None, None) == -2 and L.vc_compare_summary(None, None, None, None, None, None, None, None) == -2
    assert L.vc_compare_rings(None, 8, None, None, None, None) == -2 and L.vc_time_compare(None, 1, None) == -2
    L.vc_comparer_destroy(None)


def test_no_cpu_fallback_without_device():
    if _have_gpu():
        pytest.skip("GPU present")
    assert _create("poly3", uc.gt("poly3"), "kb4", uc.gt("kb4"), (640, 480), (64, 48)) == -1        # VC_ERR_NO_DEVICE
    assert _create("poly3", uc.gt("poly3"), "kb4", uc.gt("kb4"), (4096, 4096), (2048, 2048)) == -1   # exactly 2^22 samples is allowed
    with pytest.raises(lib.VicalibError):
        Comparer(("poly3", uc.gt("poly3")), ("kb4", uc.gt("kb4")), (640, 480))


# ---------------------------------------------------------------------------------------------------------------- the command line
def _cli(*args):
    return subprocess.run([BIN] + list(args), capture_output=True, text=True, timeout=120)


def _rigs(tmp_path):
    Ta, Tb = rc.hand_rig()
    a, b = tmp_path / "a.xml", tmp_path / "b.xml"
    a.write_text(cc.rig_xml([("poly3", uc.gt("poly3"), Ta), ("kb4", uc.gt("kb4"), Tb)]))
    b.write_text(cc.rig_xml([("poly3", uc.gt("poly3") + np.array([0, 0, 3.0, -2.0, 0, 0, 0]), Ta), ("kb4", uc.gt("kb4"), Tb)], robotics=True))
    return a, b


def test_cli_flag_errors(tmp_path):
    a, b = _rigs(tmp_path)
    both, out = "%s,%s" % (a, b), str(tmp_path / "cmp")
    for args, word in ((["-compare_models", both], "compare_dir"),
                       (["-compare_models", str(a), "-compare_dir", out], "compare_models"),
                       (["-compare_models", both + "," + str(a), "-compare_dir", out], "compare_models"),
                       (["-compare_models", both, "-compare_dir", out, "-compare_grid", "64"], "compare_grid"),
                       (["-compare_models", both, "-compare_dir", out, "-compare_grid", "1x48"], "compare_grid"),
                       (["-compare_models", both, "-compare_dir", out, "-compare_grid", "4096x4096"], "compare_grid"),
                       (["-compare_models", both, "-compare_dir", out, "-compare_grid", "641x48"], "compare_grid"),
                       (["-compare_models", both, "-compare_dir", out, "-compare_fit_radius", "0"], "compare_fit_radius"),
                       (["-compare_models", both, "-compare_dir", out, "-compare_rings", "65"], "compare_rings"),
                       (["-compare_models", both, "-compare_to", str(b), "-compare_dir", out], "exclude"),
                       (["-compare_to", str(b)], "compare_dir"),
                       (["-compare_to", str(b), "-compare_dir", out], "No camera URI")):
        r = _cli(*args)
        assert r.returncode == 1 and word in r.stderr, (args, r.returncode, r.stderr[-300:])
        assert not os.path.exists(out)


def test_cli_rig_file_errors(tmp_path):
    a, b = _rigs(tmp_path)
    out = str(tmp_path / "cmp")
    good = a.read_text()
    one = cc.rig_xml([("poly3", uc.gt("poly3"), rc.IDENTITY_POSE)])
    small = cc.rig_xml([("poly3", uc.gt("poly3"), rc.hand_rig()[0]), ("kb4", uc.gt("kb4"), rc.hand_rig()[1])], size=(320, 240))
    bad = {"missing": None, "empty": "<rig>\n</rig>\n", "type": good.replace("calibu_fu_fv_u0_v0_kb4", "calibu_unknown"),
           "params": good.replace("<params> [ 260;", "<params> [ 1; 260;"), "pose": good.replace("<T_wc> [ ", "<T_wc> [ 0.5, ", 1),
           "skew": good.replace("<T_wc> [ ", "<T_wc> [ 1.5 ", 1).replace("<T_wc> [ 1.5 0", "<T_wc> [ 1.5"), "unclosed": good.replace("</camera>\n</rig>", "</rig>"),
           "count": one, "size": small}
    for name, text in bad.items():
        p = tmp_path / (name + ".xml")
        if text is not None:
            p.write_text(text)
        for pair in ("%s,%s" % (p, b), "%s,%s" % (b, p)):
            r = _cli("-compare_models", pair, "-compare_dir", out)
            assert r.returncode == 1 and (r.stderr.startswith("F ") or "\nF " in r.stderr or "E comparison failed" in r.stderr), (name, r.returncode, r.stderr[-300:])
            assert not os.path.exists(os.path.join(out, "compare_summary.csv")), name
    r = _cli("-compare_to", str(tmp_path / "missing.xml"), "-compare_dir", out, "-cam", "detections://none.csv")
    assert r.returncode == 1 and "cannot open rig file" in r.stderr


def test_cli_without_a_device(tmp_path):
    if _have_gpu():
        pytest.skip("GPU present")
    a, b = _rigs(tmp_path)
    r = _cli("-compare_models", "%s,%s" % (a, b), "-compare_dir", str(tmp_path / "cmp"))
    assert r.returncode == 3 and "no HIP device" in r.stderr, (r.returncode, r.stderr[-300:])


def test_cli_compare_to_is_checked_before_the_solve(tmp_path):
    """a file of two cameras against a one-camera calibration, or of another image size: exit status 1 before a device is looked for"""
    a, b = _rigs(tmp_path)
    det = tmp_path / "cam0.csv"
    det.write_text("".join("%d,%d,%g,%g,%g,%g,0\n" % (f, k, 100 + 10 * k, 90 + 7 * k, 0.03 * k, 0.02 * (k % 3)) for f in range(3) for k in range(8)))
    small = tmp_path / "small.xml"
    small.write_text(cc.rig_xml([("poly3", uc.gt("poly3"), rc.IDENTITY_POSE)], size=(320, 240)))
    for rig, word in ((b, "cameras"), (small, "image sizes")):
        r = _cli("-cam", "detections://%s" % det, "-models", "poly3", "-nocalibrate_imu", "-output", str(tmp_path / "o.xml"), "-compare_to", str(rig),
                 "-compare_dir", str(tmp_path / "cmp"))
        assert r.returncode == 1 and "-compare_to" in r.stderr and word in r.stderr, (r.returncode, r.stderr[-300:])
