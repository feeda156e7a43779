"""Time of one target step (vc_target_refine_batch).
Case 1: 20 views of a 9 x 6 board at 30 mm by a linear camera (f = 420 px), tilts of 0.1 to 0.6 rad at 0.35 to 0.55 m, the board bowed and
mis-scaled as in tests/target_refine_cases.py (P = 54, D = 4).
Case 2: the views of the first 2000 frames of BASELINE cfg3's trajectory (small grid, one kb4 camera, up to 190 dots per view: P = 190, D = 8) at
the true camera and poses, the measurements of the generator (nominal board, its noise).
Device: the six stages by HIP events between them (vc_time_target_refine_batch, mean of 5 runs of the whole step after one that warms up) and the
whole call (lists built on the host, allocation, uploads, kernels, read-back: a host clock around it, best of 3 after one call that warms up).
Host: the one-thread build of the same arithmetic (tests/host_harness/target_refine_harness.cpp: an unblocked Cholesky) on the same input, once.
Nothing is asserted: the figures go into DESIGN 4.22 and profiles/README.md.
   python tools/target_refine_timing.py [n_frames] > profiles/target_refine_timing.txt"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from vicalib_amd import synth
from vicalib_amd.lib import target_refine_batch, time_target_refine_batch
import select_cases as sc
import target_refine_cases as tc


def measure(label, case):
    args = tc.lib_args(case)
    res = target_refine_batch(**args)
    wall = []
    for _ in range(3):
        t0 = time.time(); target_refine_batch(**args); wall.append(time.time() - t0)
    ms = time_target_refine_batch(**args, reps=5)
    t0 = time.time(); rc, host = tc.host_step(case); t_host = time.time() - t0
    n_corners = int(args["tile_off"][-1])
    print("%s: %d frames, %d corners, P = %d, D = %d; stages [ms] %s, sum %.3f ms; whole call %.1f ms; one-thread host build %.0f ms; status %d, gauge rank %d, "
          "%d points refined, cost %.6g, predicted decrease %.6g, |d| max %.3e m; device against host build %.2e m"
          % (label, len(case["poses"]), n_corners, len(case["points"]), sum(len(c[1]) if c[3] & 4 else 0 for c in case["cameras"]) + sum(3 * bin(c[3] & 3).count("1") for c in case["cameras"]),
             ", ".join("%s %.3f" % kv for kv in ms.items()), sum(ms.values()), 1e3 * min(wall), 1e3 * t_host, res["result_status"], res["gauge_rank"],
             int((res["point_status"] == 0).sum()), res["cost"], res["predicted_decrease"], np.abs(res["refined"] - case["points"]).max(),
             np.abs(res["refined"] - host["refined"]).max() if rc == 0 else float("nan")))


rng = np.random.default_rng(3)
ii, jj = np.meshgrid(np.arange(9), np.arange(6), indexing="xy")
nominal = np.stack([(ii.ravel() - 4) * 0.03, (jj.ravel() - 2.5) * 0.03, np.zeros(54)], axis=1)
cams = [("linear", [420.0, 420.0, 319.5, 239.5], synth.se3_from_Rt(np.eye(3), np.zeros(3)), 4)]
poses = np.stack([sc.pose(rng, dist=(0.35, 0.55), tilt=0.6, shift=0.02) for _ in range(20)])
true = nominal + tc.defects(nominal)
tiles = [(f, 0, np.arange(54), tc.measure(cams, poses, true, f, 0, np.arange(54), rng, 0.05)) for f in range(20)]
measure("board 9 x 6", dict(cameras=cams, poses=poses, tiles=tiles, points=nominal, nominal=nominal, lam=1e4))

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
cfg = synth.BASELINE_CONFIGS["cfg3"]
p = synth.generate(synth.Config(models=("kb4",), grid=cfg.grid, n_frames=n, imu=True))
cams = [("kb4", list(p.cam_K_gt[0]), p.cam_T_ck_gt[0], 4)]
measure("cfg3", dict(cameras=cams, poses=np.asarray(p.frame_T_wk_gt), tiles=[(t[0], t[1], t[2], t[3]) for t in p.tiles], points=np.asarray(p.grid_points),
                     nominal=np.asarray(p.grid_points), lam=1e4))
