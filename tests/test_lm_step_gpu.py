"""One LM step of the device pass against a dense reference solve (tests/lm_step_ref.py), at one fixed linearisation point.

vc_step_hold runs a pass with the decision withheld and reads out what it formed: the damping of the frames and of the shared parameters,
the step of the shared parameters (k_reduced: the one-wavefront solve at D <= 32, the register-tiled one above) and the trial state (the
back-substitution of the frames -- k_trial / k_backsub on vision-only passes, the chain's back-substitution with the IMU -- and the manifold
update).  The reference is the oracle's linearisation at the same state with the same weights, its damping (vco_lm_lambda, as solve_once
forms it) and a dense solve with iterative refinement.  For each radius:
  - damping: equal to 1e-12 relative;
  - delta_s: || (delta_s,dev - delta_s,ref) / s || <= C_BOUND(n) * eps * kappa(M~) * || x~_ref || (lm_step_ref: Jacobi-scaled coordinates,
    x~_ref the whole scaled step, frames included);
  - trial state: every block (a frame's pose, its velocity, a camera, the IMU parameters) within (1 + |x|) * 2 max(s of the block) times
    that bound of the reference trial state (vco_apply_step of the reference step), plus 16 eps |x| for the update's own rounding.
Radius 1e0 is the heavily damped first pass (every bound <= 1e-9 there), 1e4 the first pass of every solve, 1e8 close to Gauss-Newton.
Every case asserts the width of its reduced system and, with the IMU, the forms of the pass it ran (vc_pass_paths).  Environment switches
run in a child process each (python lm_step_ref.py <case>), one at a time."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import oracle_lib as ol          # noqa: E402
import lm_step_ref as ref        # noqa: E402
from vicalib_amd import synth    # noqa: E402
from vicalib_amd.lib import ViCalibrator      # noqa: E402

pytestmark = pytest.mark.gpu
RADII = (1e0, 1e4, 1e8)
EPS = np.finfo(np.float64).eps
ALL_FLAGS = (True, True, False, True)
PATH_KEYS = ("fold_l0", "back_path", "tail_deferred", "shared_blocks_ahead")


def _v(models, n_frames, D, seed=37, fix=False, drop=None, env=None):
    return dict(kind="vision", models=models, n_frames=n_frames, D=D, seed=seed, fix=fix, drop=drop, env=env or {})


def _i(models, n_frames, D, flags=ALL_FLAGS, seed=5, paths=None, env=None, init=False):
    return dict(kind="vi", models=models, n_frames=n_frames, D=D, seed=seed, flags=flags, paths=paths, env=env or {}, init=init)


ON = dict(fold_l0=1, back_path=1, shared_blocks_ahead=1)
CASES = {
    # one-wavefront reduced solve, vision only
    "mono_poly3": _v(("poly3",), 12, 7),
    "stereo_fov_kb4": _v(("fov", "kb4"), 20, 19),
    "stereo_fixed_intrinsics": _v(("fov", "kb4"), 20, 6, fix=True),
    "frame_without_detections": _v(("poly3", "fov"), 12, 18, drop=3),
    # register-tiled reduced solve, vision only (3, 4, 4, 5, 7, 7, 8 row tiles of 16)
    "tiled_36": _v(("kb4",) * 3, 30, 36),
    "tiled_50": _v(("kb4",) * 4, 30, 50),
    "tiled_59": _v(("poly3",) * 5, 30, 59),
    "tiled_78": _v(("kb4",) * 6, 30, 78),
    "tiled_102": _v(("poly3", "kb4") * 4, 30, 102),
    "tiled_106": _v(("kb4",) * 8, 30, 106),
    "tiled_122": _v(("rational6",) * 8, 30, 122),
    "pre_backsub_40": _v(("fov", "kb4"), 40, 19, env=dict(VICALIB_AMD_PRE_BACKSUB="1")),
    # chain elimination with the IMU, at the widths of the reduced solve
    "vi_linear_25": _i(("linear",), 40, 25),
    "vi_kb4_29": _i(("kb4",), 40, 29),
    "vi_rational6_31": _i(("rational6",), 40, 31),
    "vi_32": _i(("poly3", "rational6"), 21, 32, flags=(False, True, False, True)),
    "vi_cfg4_rig_67": _i(("poly3",) * 4, 66, 67),
    "vi_cfg5_rig_115": _i(("fov", "kb4") * 4, 66, 115),
    # chain structure: frame counts on every side of the group boundaries
    "vi_kb4_7": _i(("kb4",), 7, 29),
    "vi_kb4_9": _i(("kb4",), 9, 29),
    "vi_kb4_57": _i(("kb4",), 57, 29),
    "vi_kb4_64": _i(("kb4",), 64, 29),
    "vi_kb4_65": _i(("kb4",), 65, 29),
    "vi_kb4_130": _i(("kb4",), 130, 29, paths=ON),
    # the alternative forms of the pass, each against the same reference
    "vi_kb4_130_back_levels": _i(("kb4",), 130, 29, paths=dict(back_path=0), env=dict(VICALIB_AMD_BACK_PATH="0")),
    "vi_kb4_130_no_fold": _i(("kb4",), 130, 29, paths=dict(fold_l0=0), env=dict(VICALIB_AMD_FOLD_L0="0")),
    "vi_kb4_130_no_hadd": _i(("kb4",), 130, 29, paths=dict(shared_blocks_ahead=0), env=dict(VICALIB_AMD_HADD_EARLY="0")),
    # three levels below the top: the reduced solve's tail rides in the back-substitution's launch
    "vi_kb4_520": _i(("kb4",), 520, 29, paths=dict(ON, tail_deferred=1)),
    "vi_kb4_520_no_defer": _i(("kb4",), 520, 29, paths=dict(tail_deferred=0), env=dict(VICALIB_AMD_DEFER_TAIL="0")),
    # optimisation flags
    "vi_rotation_only": _i(("fov", "kb4"), 21, 35, flags=(True, True, True, True), init=True),
    "vi_no_time_offset": _i(("fov", "kb4"), 21, 39, flags=(True, True, False, False)),
    "vi_biases_inactive": _i(("fov", "kb4"), 21, 28, flags=(False, True, False, True)),
}


def _setup(case):
    """(calibrator, oracle, df) at the case's linearisation point, both sides with the same multiplicities and IMU weights."""
    if case["kind"] == "vision":
        p = synth.generate(synth.Config(models=case["models"], n_frames=case["n_frames"], seed=case["seed"]))
        if case["drop"] is not None:
            p.tiles = [t for t in p.tiles if t[0] != case["drop"]]
        cal = ViCalibrator(0).load_problem(p)
        cal.SetCalibrateImu(False)
        orc = ol.Oracle().load(p); orc.set_options(calibrate_imu=False, fix_intrinsics=case["fix"])
        if case["fix"]:
            cal.FixCameraIntrinsics(True)
        orc.prepare(vis_mult=1)
        cal.prepare()
        return cal, orc, 6
    p = synth.generate(synth.Config(models=case["models"], n_frames=case["n_frames"], imu=True, seed=case["seed"]))
    gt = p.imu_gt
    b0 = np.concatenate([gt["bg"], gt["ba"]]) * 0.7; s0 = np.concatenate([gt["sg"], gt["sa"]]) * 1.005; g0 = np.array([0.02, 0.01])
    cal = ViCalibrator(0).load_problem(p, init=case["init"])
    orc = ol.Oracle().load(p, init=case["init"]); orc.set_options(calibrate_imu=True)
    orc.set_flags(*case["flags"]); orc.set_imu_state(b0, s0, g0, 0.0013)
    cal.SetOptimizationFlags(*case["flags"]); cal.SetBiases(b0); cal.SetScaleFactor(s0); cal.SetTimeOffset(0.0013); cal.SetGravity(g0)
    orc.prepare(vis_mult=1, imu_mult=1)
    # every pass updates weight_sqrt_ at the accepted state for the next one (the update is pinned by test_gpu_parity's weight tests):
    # one pass first, then both sides linearise with the weights it left
    cal.linearize()
    orc.set_imu_weights(cal.imu_weights())
    return cal, orc, orc.layout()["df"]


def _block_check(what, dev, want, x0, smax, E):
    """|dev - want| of one block of the trial state against (1 + |x|) 2 smax E + 16 eps |x|."""
    xm = max(np.abs(x0).max(), np.abs(want).max())
    allow = (1.0 + xm) * 2.0 * smax * E + 16.0 * EPS * xm
    err = np.abs(np.asarray(dev) - np.asarray(want)).max()
    assert err <= allow, f"{what}: |trial - reference| = {err:.3e} > {allow:.3e}"
    return err / allow if allow > 0 else 0.0


def check_case(case, child=False):
    if case["env"] and not child:
        env = dict(os.environ); env.update(case["env"])
        name = [k for k, v in CASES.items() if v is case][0]
        r = subprocess.run([sys.executable, os.path.join(HERE, "lm_step_ref.py"), name], env=env, capture_output=True, text=True, timeout=600)
        print(r.stdout)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert ("ok " + name) in r.stdout
        return
    cal, orc, df = _setup(case)
    D = cal.shared_dim()
    assert D == case["D"], (D, case["D"])
    if case["kind"] == "vi":
        paths = cal.pass_paths()
        print("pass paths", paths)
        for k, v in (case["paths"] or {}).items():
            assert paths[k] == v, (k, paths)
    lin = orc.linearize()
    n = lin["A"].shape[0]
    assert lin["Hss"].shape[0] == D
    T0, v0 = orc.frames()
    cams0 = [orc.camera(c) for c in range(orc.n_cams)]
    imu0 = orc.imu_state()
    for radius in RADII:
        got = cal.step_hold(radius)
        assert abs(got["cost"] - lin["cost"]) <= 1e-10 * abs(lin["cost"])      # same state, same weights
        lam = orc.lm_lambda(radius)
        r = ref.reference_step(lin, lam, df)
        print(f"radius {radius:g}: n = {r['n']}, kappa(M~) = {r['kappa']:.3e}, bound = {r['rel']:.3e}")
        if radius == 1e0:
            assert r["rel"] <= 1e-9, "badly chosen case: the heavily damped pass must be well conditioned"
        s = r["scale"]; ss = s[n * df:]
        act_f = r["active"][:n * df].reshape(n, df).all(axis=1)
        # damping
        np.testing.assert_allclose(got["slam"], lam[n * 9:], rtol=1e-12)
        np.testing.assert_allclose(got["frame_lam"][act_f, :df], lam[:n * 9].reshape(n, 9)[act_f, :df], rtol=1e-12)
        # delta_s
        xn = ref.scaled_norm(r, r["dfv"], r["dsv"])
        E = r["rel"] * xn
        es = float(np.linalg.norm((got["delta_s"] - r["dsv"]) / ss))
        print(f"  |delta_s error|~ / |x~_ref| = {es / xn:.3e}")
        assert es <= E, f"delta_s: scaled error {es / xn:.3e} of the step > bound {r['rel']:.3e}"
        # trial state against the oracle's update with the reference step
        orc.apply_step(r["dfv"], r["dsv"])
        T1, v1 = orc.frames()
        cams1 = [orc.camera(c) for c in range(orc.n_cams)]
        imu1 = orc.imu_state()
        for f in range(n):
            sf = s[f * df:(f + 1) * df]
            _block_check(f"frame {f} pose", got["poses"][f], T1[f], T0[f], sf[:6].max(), E)
            if df == 9:
                _block_check(f"frame {f} velocity", got["vels"][f], v1[f], v0[f], sf[6:9].max(), E)
        lay = orc.layout()
        for c in range(orc.n_cams):
            cols = [lay["cam"][c][0] + k for k in range(3)] if lay["cam"][c][0] >= 0 else []
            cols += [lay["cam"][c][1] + k for k in range(3)] if lay["cam"][c][1] >= 0 else []
            nk = len(cams1[c][0])
            cols += [lay["cam"][c][2] + k for k in range(nk)] if lay["cam"][c][2] >= 0 else []
            smax = ss[cols].max() if cols else 0.0
            _block_check(f"camera {c} T_ck", got["cams"][c][:7], cams1[c][1], cams0[c][1], smax, E)
            _block_check(f"camera {c} intrinsics", got["cams"][c][7:7 + nk], cams1[c][0], cams0[c][0], smax, E)
        if case["kind"] == "vi":
            b1, sf1, g1, t1 = imu1
            b0, sf0, g0, t0 = imu0
            for what, off, dev, want, x0 in (("gravity", lay["g"], got["imus"][0:2], g1, g0), ("biases", lay["b"], got["imus"][2:8], b1, b0),
                                             ("scale factors", lay["sf"], got["imus"][8:14], sf1, sf0), ("time offset", lay["toff"], got["imus"][14:15], [t1], [t0])):
                k = len(want)
                smax = ss[off:off + k].max() if off >= 0 else 0.0
                _block_check(what, dev, want, x0, smax, E)
        # back to the linearisation point for the next radius
        for f in range(n):
            orc.set_frame(f, T0[f], v0[f])
        for c in range(orc.n_cams):
            orc.set_camera(c, cams0[c][0], cams0[c][1])
        orc.set_imu_state(imu0[0], imu0[1], imu0[2], imu0[3])


@pytest.mark.parametrize("name", list(CASES))
def test_lm_step_matches_dense_reference_solve(name):
    check_case(CASES[name])
