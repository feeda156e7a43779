"""Time of the pose seeds on the device next to the host routine they replace.
The views of the first 2000 frames of BASELINE cfg3's trajectory (small grid, one kb4 camera at ground truth, up to 190 corners per view), plain
and with 100 minimal-sample iterations at 1 px.  Device: the kernel of vc_pnp_planar_batch alone (vc_time_pnp_planar_batch: HIP events,
launches back to back) and the whole call (allocation, uploads, kernel, read-back: a host clock around it, best of 3 after one call that warms
up).  Calibrator: vc_init_frame_poses_pnp of one calibrator holding the same views, with vc_set_pnp_device off (the host routine, one thread) and
on.  No speed-up is asserted anywhere: the figures go into DESIGN 4.15 and profiles/README.md.
   python tools/seed_timing.py [n_frames]"""
import os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from vicalib_amd import synth
from vicalib_amd.lib import ViCalibrator, pnp_planar_batch, time_pnp_planar_batch

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
cfg = synth.BASELINE_CONFIGS["cfg3"]
p = synth.generate(synth.Config(models=("kb4",), grid=cfg.grid, n_frames=n, imu=True))
tiles = p.tiles
off = np.concatenate([[0], np.cumsum([len(t[2]) for t in tiles])]).astype(np.int32)
pw = np.concatenate([p.grid_points[t[2]] for t in tiles]); pc = np.concatenate([t[3] for t in tiles])
models, params = ["kb4"] * len(tiles), [p.cam_K_gt[0]] * len(tiles)
print("%d views, %d corners (%d .. %d per view)" % (len(tiles), len(pw), np.diff(off).min(), np.diff(off).max()))
cal = ViCalibrator(0)
cal.AddCamera("kb4", p.cam_K_gt[0], p.cam_T_ck_gt[0], p.cfg.width, p.cfg.height)
for f in range(len(p.frame_time)):
    cal.AddFrame(p.frame_T_wk_init[f], p.frame_time[f])
for (f, c, ids, pix) in tiles:
    cal.AddObservations(f, c, p.grid_points[ids], pix)
for label, its, tol in (("plain", 0, 0.0), ("100 iterations at 1 px", 100, 1.0)):
    res = pnp_planar_batch(models, params, off, pw, pc, iterations=its, tol_px=tol)
    wall = []
    for _ in range(3):
        t0 = time.time(); pnp_planar_batch(models, params, off, pw, pc, iterations=its, tol_px=tol); wall.append(time.time() - t0)
    ms = time_pnp_planar_batch(models, params, off, pw, pc, iterations=its, tol_px=tol, reps=10)
    print("%s: kernel %.3f ms (%.2f us per view); whole call %.1f ms; status %s; mean inliers %.1f; mean rms %.4f px"
          % (label, ms, 1e3 * ms / len(tiles), 1e3 * min(wall), np.bincount(res["status"], minlength=5).tolist(), res["n_inliers"].mean(), res["rms"].mean()))
    cal.SetPnPRansac(its, tol)
    took = {}
    for on in (True, False):
        cal.SetPnPDevice(on)
        if on:
            cal.InitFramePosesPnP()          # (warms up)
        took[on] = float("inf")
        for _ in range(3 if on else 1):      # (best of 3 on the device; the host routine runs for seconds: once)
            t0 = time.time(); seeded = cal.InitFramePosesPnP(); took[on] = min(took[on], time.time() - t0)
    print("%s: vc_init_frame_poses_pnp of %d frames (%d seeded): device path %.1f ms, host routine on one thread %.1f ms"
          % (label, len(p.frame_time), seeded, 1e3 * took[True], 1e3 * took[False]))
