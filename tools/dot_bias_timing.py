"""Time of the predicted centre bias of every dot observation (vc_dot_bias_batch).
Case 1: the views of the first 2000 frames of BASELINE cfg3's trajectory (small grid, one kb4 camera, up to 190 dots per view; the input of
tools/seed_timing.py) at the true camera and poses, the preset's radii (4.23 / 2.83 mm by a generated pattern).
Case 2: the 20 views of the command-line test (tests/dot_bias_cli_case.py: a linear camera, 54 dots per view).
Device: the kernel alone (vc_time_dot_bias_batch: HIP events, launches back to back) and the whole call (allocation, uploads, kernel, read-back:
a host clock around it, best of 3 after one call that warms up).  Host: the one-lane build of the same arithmetic
(tests/host_harness/dot_bias_harness.cpp) on the same input, one thread, best of 3.
Nothing is asserted: the figures go into DESIGN 4.20 and profiles/README.md.
   python tools/dot_bias_timing.py [n_frames] > profiles/dot_bias_timing.txt"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from vicalib_amd import synth
from vicalib_amd.lib import dot_bias_batch, time_dot_bias_batch, target_make_pattern
import dot_bias_cases as dc
import dot_bias_cli_case as case


def se3_mul_inv(T_ck, T_wk):
    """T_cw = T_ck T_wk^-1"""
    Rck, Rwk = synth.quat_to_matrix(T_ck[:4]), synth.quat_to_matrix(T_wk[:4])
    Rcw = Rck @ Rwk.T
    return synth.se3_from_Rt(Rcw, T_ck[4:] - Rcw @ T_wk[4:])


def measure(label, arrays):
    n_views, n = len(arrays[0]), len(arrays[5])
    res = dot_bias_batch(*arrays)
    wall = []
    for _ in range(3):
        t0 = time.time(); dot_bias_batch(*arrays); wall.append(time.time() - t0)
    ms = time_dot_bias_batch(*arrays, reps=10)
    host = []
    dc.host_run(arrays)
    for _ in range(3):
        t0 = time.time(); hres = dc.host_run(arrays); host.append(time.time() - t0)
    ok = res["status"] == 0
    both = ok & (hres["status"] == 0)
    print("%s: %d views, %d observations; kernel %.4f ms (%.2f ns per observation); whole call %.2f ms; one-lane host build %.1f ms; status %s; "
          "bias rms %.4f px, max %.4f px; radius %.2f .. %.2f px; device against host build %.2e px"
          % (label, n_views, n, ms, 1e6 * ms / n, 1e3 * min(wall), 1e3 * min(host), np.bincount(res["status"], minlength=5).tolist(),
             np.sqrt(np.mean(np.sum(res["bias"][ok] ** 2, axis=1))), np.sqrt(np.sum(res["bias"][ok] ** 2, axis=1)).max(), res["radius_px"][ok].min(),
             res["radius_px"][ok].max(), np.abs(res["bias"][both] - hres["bias"][both]).max()))


n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
cfg = synth.BASELINE_CONFIGS["cfg3"]
p = synth.generate(synth.Config(models=("kb4",), grid=cfg.grid, n_frames=n, imu=True))
gw, gh, _ = synth.GRIDS[cfg.grid]
radius_by_dot = np.where(target_make_pattern(gh, gw).ravel() == 1, 0.00423, 0.00283)
off = np.concatenate([[0], np.cumsum([len(t[2]) for t in p.tiles])]).astype(np.int32)
measure("cfg3", (["kb4"] * len(p.tiles), [p.cam_K_gt[0]] * len(p.tiles), np.array([se3_mul_inv(p.cam_T_ck_gt[t[1]], p.frame_T_wk_gt[t[0]]) for t in p.tiles]), off,
                 np.concatenate([p.grid_points[t[2]] for t in p.tiles]), np.concatenate([radius_by_dot[t[2] % len(radius_by_dot)] for t in p.tiles])))

c = case.build()
rng = np.random.default_rng(3)
T = []
for v in range(case.N_VIEWS):          # (poses of the case's kind; the timing does not depend on which)
    rot = np.append(rng.standard_normal(2), 0.0); rot *= rng.uniform(0.1, 0.6) / np.linalg.norm(rot)
    T.append(dc.pose(rot, -synth.so3_exp_matrix(rot) @ c["P"].mean(axis=0) + np.array([0.0, 0.0, rng.uniform(0.35, 0.55)])))
measure("20 views", (["linear"] * case.N_VIEWS, [case.K_TRUE] * case.N_VIEWS, np.array(T), np.arange(case.N_VIEWS + 1, dtype=np.int32) * len(c["P"]),
                     np.tile(c["P"], (case.N_VIEWS, 1)), np.tile(c["radius"], case.N_VIEWS)))
