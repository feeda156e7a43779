"""Mapping the row and depth uncertainty of a calibrated stereo pair (vc_stereo_uncertainty*), the part that needs no GPU: the map's arithmetic
(vc_stereo_uncertainty.hpp, rect_pose_jacobian) compiled for the host and held to the same numpy reference and the same checks that
tests/test_stereo_uncertainty_gpu.py applies to the kernels, the semantic pin against numpy's re-rectification of the fixed pixels, the exact
properties, argument errors, the refusal to run without a device, and the command line's flag errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rectify_cases as rc
import stereo_uncertainty_cases as su
import undistort_cases as uc
import vicalib_amd.lib as lib
from vicalib_amd import synth

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
    src = os.path.join(HERE, "host_harness", "stereo_uncertainty_harness.cpp")
    so = os.path.join(HERE, "host_harness", "libvc_stereo_uncertainty_harness.so")
    deps = [src] + [os.path.join(ROOT, "vicalib_amd", "csrc", f) for f in ("vc_stereo_uncertainty.hpp", "vc_uncertainty.hpp", "vc_convert.hpp", "vc_lm_rules.hpp",
                                                                          "vc_compare.hpp", "vc_rectify.hpp", "vc_undistort.hpp", "vc_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def host_pose_jacobian(T_ck_a, T_ck_b):
    W = np.zeros((7, 12))
    return _harness().vch_su_pose_jacobian(_p(_d(T_ck_a)), _p(_d(T_ck_b)), _p(W)), W


def host_stereo_uncertainty(cameras, T_ck, cov, sigma_px=1.0, depths=su.DEPTHS, grid=su.GRID, dl=su.DST_LINEAR, size=su.SIZE):
    """the host build of a whole run; (status, dict in the layout the checks take)"""
    (ma, Ka), (mb, Kb) = cameras
    Ka, Kb, Ta, Tb, cov, dl, depths = _d(Ka), _d(Kb), _d(T_ck[0]), _d(T_ck[1]), _d(cov), _d(dl), _d(depths)
    n, nd = grid[0] * grid[1], len(depths)
    var, fl, summary, pose_var = np.zeros((max(nd, 1), n, 3)), np.zeros((max(nd, 1), n), dtype=np.uint8), np.zeros((max(nd, 1), 7)), np.zeros(7)
    st = _harness().vch_stereo_uncertainty(synth.MODEL_IDS[ma], _p(Ka), len(Ka), size[0], size[1], _p(Ta), synth.MODEL_IDS[mb], _p(Kb), len(Kb), size[0], size[1], _p(Tb),
                                           _p(dl), size[0], size[1], grid[0], grid[1], _p(cov), C.c_double(sigma_px), _p(depths), nd, _p(var), _p(fl), _p(summary), _p(pose_var))
    if st != 0:
        return st, None
    _, W = host_pose_jacobian(Ta, Tb)
    keys = ("count", "invalid", "sum_var_dv", "sum_var_d", "sum_var_z", "max_var_dv", "worst")
    return 0, dict(var=var, flags=fl, pose_var=pose_var, W=W,
                   summary=[{k: (int(v) if k in ("count", "invalid", "worst") else float(v)) for k, v in zip(keys, row)} for row in summary])


def host_run(c, cov, sigma_px, depths, **kw):
    st, out = host_stereo_uncertainty(c.cameras, c.T_ck, cov, sigma_px, depths, grid=c.grid, **kw)
    assert st == 0
    return out


def host_args_ok(cov, sigma_px=1.0, depths=su.DEPTHS):
    cov, depths = _d(cov), _d(depths)
    return bool(_harness().vch_su_args_ok(_p(cov), len(cov), C.c_double(sigma_px), _p(depths), len(depths)))


# ---------------------------------------------------------------------------------------------------------------- the cases' own conditions
@pytest.mark.parametrize("pair", su.MODEL_PAIRS + ("left",))
def test_every_full_lattice_case_has_valid_and_invalid_samples(pair):
    su.check_shares(su.reference(pair if pair == "left" else "%s-%s" % pair))


# ---------------------------------------------------------------------------------------------------------------- checks 1 and 2 on the host build
_deviations = {}


@pytest.mark.parametrize("name", su.case_names())
def test_host_arithmetic(name):
    _, dev = su.check_case(name, host_run)
    _deviations[name] = dev
    print("largest relative deviation of the host harness from numpy so far: %.3g (stereo_uncertainty_cases.MEASURED = %.3g)" % (max(_deviations.values()), su.MEASURED))


@pytest.mark.parametrize("rig", ("hand", "hand-left", "fov-fov", "kb4-poly3"))
def test_pose_jacobian_against_central_differences(rig):
    Ta, Tb = rc.rigs()[rig]
    st, W = host_pose_jacobian(Ta, Tb)
    assert st == 0
    ref, num = su.numpy_pose_jacobian(Ta, Tb), su.numeric_pose_jacobian(Ta, Tb)
    scale = np.abs(num).max(axis=1, keepdims=True)
    print("%s: W against numpy %.3g, against central differences %.3g of the row's largest entry" % (rig, (np.abs(W - ref) / scale).max(), (np.abs(W - num) / scale).max()))
    assert (np.abs(W - ref) / scale).max() <= su.TOLERANCE
    assert (np.abs(W - num) / scale).max() <= 1e-8 and (np.abs(ref - num) / scale).max() <= 1e-8      # (Richardson at h = 1e-4: h^4 and the rounding 1e-16 / h)
    # through the library itself
    W2 = np.zeros((7, 12))
    assert lib.load().vc_stereo_pose_jacobian(_p(_d(Ta)), _p(_d(Tb)), _p(W2)) == 0 and np.array_equal(W2, W)


# ---------------------------------------------------------------------------------------------------------------- check 3: the semantic pin
@pytest.mark.parametrize("what,k,delta,tab_dv,tab_d", su.PIN)
def test_rank_one_covariance_is_the_re_rectified_shift(what, k, delta, tab_dv, tab_d):
    planes, gaps = su.pin_numpy(what, k, delta)
    _, half = su.pin_numpy(what, k, 0.5 * delta)
    print("%s %d: gaps %s px at delta, %s px at delta / 2: ratios %s" % (what, k, gaps, half, gaps / half))
    assert np.all(gaps / half >= 3.5) and np.all(gaps / half <= 4.5)                 # second order in delta
    c = su.case("%s-%s" % su.PIN_PAIR)
    _, _, cov = su.pin_perturbed(what, k, delta)
    su.check_pin(what, k, delta, (tab_dv, tab_d), host_run(c, cov, 1.0, c.depths), planes, gaps)


# ---------------------------------------------------------------------------------------------------------------- check 4: exact properties
def test_exact_properties_on_the_host_build():
    c = su.case("kb4-poly3")
    one = host_run(c, c.cov, 1.0, c.depths)
    zero = host_run(c, np.zeros_like(c.cov), 1.0, c.depths)
    good = (one["flags"] & su.FLAG_INVALID) == 0
    assert not np.any(zero["var"][good]) and np.array_equal(zero["flags"], one["flags"]) and not np.any(zero["pose_var"])
    assert all(s["sum_var_dv"] == 0 and s["sum_var_z"] == 0 and s["max_var_dv"] == 0 for s in zero["summary"])
    assert su.same_bits(one, host_run(c, c.cov, 2.0, c.depths), scale=4.0)
    assert su.same_bits(one, host_run(c, c.cov, 1.0, c.depths))
    for k, Z in enumerate(c.depths):
        assert su.same_bits(su.plane(one, k), host_run(c, c.cov, 1.0, (Z,)))


def test_swapping_the_sides_keeps_the_row_variance():
    c = su.case("kb4-poly3")
    one = host_run(c, c.cov, 1.0, c.depths)
    for k, Z in enumerate(c.depths):
        cams, T, dl, cov = su.swapped(c, Z)
        st, other = host_stereo_uncertainty(cams, T, cov, 1.0, (Z,), grid=c.grid, dl=dl)
        assert st == 0
        und = su.reference(c.name).undecided[k]
        fa, fb = one["flags"][k], other["flags"][0]
        assert np.array_equal(((fa & 1) << 1 | (fa & 2) >> 1 | (fa & 4))[~und], fb[~und])
        both = ((fa | fb) & su.FLAG_INVALID) == 0
        off = np.abs(other["var"][0][both, 0] - one["var"][k][both, 0]) / one["var"][k][both, 0]
        print("depth %g: var_dv of the swapped pair off by %.3g" % (Z, off.max()))
        assert both.sum() > 0.3 * len(both) and off.max() <= su.TOLERANCE


def test_lattice_sizes():
    for name, n in (("tiny", 4), ("one-workgroup", 1024)):
        c = su.case(name)
        out = host_run(c, c.cov, 1.0, c.depths)
        assert all(s["count"] + s["invalid"] == n for s in out["summary"])


# ---------------------------------------------------------------------------------------------------------------- argument errors
def test_run_argument_errors_through_the_shared_check():
    c = su.case("kb4-poly3")
    cov = c.cov
    assert host_args_ok(cov) and host_args_ok(np.zeros_like(cov)) and host_args_ok(cov, depths=(1.0,) * 8)
    bad = cov.copy(); bad[1, 20] += 1e-9 * cov.diagonal().max()
    assert not host_args_ok(bad)                                    # not symmetric
    bad = cov.copy(); bad[3, 3] = -1e-9
    assert not host_args_ok(bad)                                    # a negative diagonal entry
    for v in (np.nan, np.inf):
        bad = cov.copy(); bad[2, 5] = bad[5, 2] = v
        assert not host_args_ok(bad)
    for s in (0.0, -1.0, np.nan, np.inf):
        assert not host_args_ok(cov, sigma_px=s)
    for d in ((0.0,), (-1.0,), (np.nan,), (np.inf,), (1.0, 2.0, -3.0), (1.0,) * 9):
        assert not host_args_ok(cov, depths=d)
    assert not _harness().vch_su_args_ok(_p(_d(cov)), len(cov), C.c_double(1.0), _p(_d([1.0])), 0)
    assert host_stereo_uncertainty(c.cameras, c.T_ck, cov, grid=(641, 48))[0] == -2 and host_stereo_uncertainty(c.cameras, c.T_ck, cov, grid=(1, 48))[0] == -2
    assert host_stereo_uncertainty(c.cameras, (c.T_ck[0], c.T_ck[0]), cov)[0] == -6                  # a coincident rig
    assert host_stereo_uncertainty(c.cameras, rc.vertical_rig(), cov)[0] == -7                       # a vertical rig
    assert host_pose_jacobian(c.T_ck[0], c.T_ck[0])[0] == 1 and host_pose_jacobian(*rc.vertical_rig())[0] == 2


def _create(cams, T_ck, dl=su.DST_LINEAR, size=su.SIZE, dst=su.SIZE, alpha=0.0, grid=(64, 48), models=None):
    (ma, Ka), (mb, Kb) = cams
    ids = models if models is not None else (synth.MODEL_IDS[ma], synth.MODEL_IDS[mb])
    Ka, Kb, Ta, Tb = _d(Ka), _d(Kb), _d(T_ck[0]), _d(T_ck[1])
    h = C.c_void_p()
    st = lib.load().vc_stereo_uncertainty_create(0, int(ids[0]), _p(Ka), len(Ka), size[0], size[1], _p(Ta), int(ids[1]), _p(Kb), len(Kb), size[0], size[1], _p(Tb),
                                                 _p(_d(dl)) if dl is not None else None, dst[0], dst[1], C.c_double(alpha), grid[0], grid[1], C.byref(h))
    if h.value:
        lib.load().vc_stereo_uncertainty_destroy(h)
    return st


def test_argument_errors_come_before_the_device():
    c = su.case("kb4-poly3")
    cams, T = c.cameras, c.T_ck
    assert _create(cams, T, models=(7, 2)) == -2 and _create(cams, T, models=(3, -1)) == -2                   # an unknown model
    assert _create((cams[0], ("poly3", c.K[1][:6])), T) == -2 and _create((("kb4", c.K[0][:7]), cams[1]), T) == -2      # a wrong nparams
    assert _create(cams, T, grid=(641, 48)) == -2 and _create(cams, T, grid=(64, 481)) == -2 and _create(cams, T, grid=(1, 48)) == -2
    assert _create(cams, T, dst=(4096, 4096), grid=(2049, 2048)) == -2       # above 2^22 samples
    bad = T[0].copy(); bad[:4] *= 1.01
    assert _create(cams, (bad, T[1])) == -2                                  # a quaternion that is not a unit one
    bad = T[1].copy(); bad[5] = np.nan
    assert _create(cams, (T[0], bad)) == -2
    assert _create(cams, T, dl=None, alpha=1.5) == -2 and _create(cams, T, dl=[300.0, np.nan, 319.5, 239.5]) == -2
    assert _create(cams, (T[0], T[0])) == -6                                 # a coincident rig: VC_ERR_NUMERIC
    assert _create(cams, rc.vertical_rig()) == -7                            # a vertical rig: VC_ERR_UNSUPPORTED
    L = lib.load()
    one = _d([1.0])
    assert L.vc_stereo_uncertainty_run(None, None, C.c_double(1.0), _p(one), 1) == -2
    assert L.vc_stereo_uncertainty_get_map(None, None, None) == -2 and L.vc_stereo_uncertainty_get_pose_sigma(None, None) == -2
    assert L.vc_stereo_uncertainty_summary(None, 0, None, None, None, None, None, None, None) == -2
    assert L.vc_stereo_uncertainty_get(None, None, None, None, None, None) == -2 and L.vc_time_stereo_uncertainty(None, 1, None) == -2
    assert L.vc_stereo_uncertainty_create_for_cameras(None, 0, 1, None, 640, 480, C.c_double(0.0), 64, 48, None) == -2
    W = np.zeros((7, 12))
    assert L.vc_stereo_pose_jacobian(_p(_d(T[0])), _p(_d(T[0])), _p(W)) == -6 and L.vc_stereo_pose_jacobian(_p(_d(T[0])), None, _p(W)) == -2
    L.vc_stereo_uncertainty_destroy(None)


def test_no_cpu_fallback_without_device():
    if _have_gpu():
        pytest.skip("GPU present")
    c = su.case("kb4-poly3")
    assert _create(c.cameras, c.T_ck) == -1                                  # VC_ERR_NO_DEVICE
    assert _create(c.cameras, c.T_ck, dl=None, alpha=0.0) == -1              # ... after the fit of the destination camera
    with pytest.raises(lib.VicalibError):
        lib.StereoUncertainty(c.cameras[0], c.cameras[1], su.SIZE, su.SIZE, c.T_ck[0], c.T_ck[1], dst_linear=su.DST_LINEAR)


# ---------------------------------------------------------------------------------------------------------------- the command line
def test_cli_flag_errors(tmp_path):
    out = str(tmp_path / "su")
    for args, word in ((["-stereo_uncertainty_grid", "64"], "stereo_uncertainty_grid"),
                       (["-stereo_uncertainty_grid", "1x48"], "stereo_uncertainty_grid"),
                       (["-stereo_uncertainty_cams", "0"], "stereo_uncertainty_cams"),
                       (["-stereo_uncertainty_cams", "1,1"], "stereo_uncertainty_cams"),
                       (["-stereo_uncertainty_depths", "1,-2"], "stereo_uncertainty_depths"),
                       (["-stereo_uncertainty_depths", "1,2,3,4,5,6,7,8,9"], "stereo_uncertainty_depths"),
                       (["-stereo_uncertainty_depths", "1,x"], "stereo_uncertainty_depths"),
                       (["-stereo_uncertainty_noise", "-1"], "stereo_uncertainty_noise")):
        r = subprocess.run([BIN, "-cam", "detections://missing.txt", "-stereo_uncertainty_dir", out] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and word in r.stderr, (args, r.returncode, r.stderr[-300:])
        assert not os.path.exists(out)
