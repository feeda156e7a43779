"""Time of the focal-length seed, and what it does to the solve it seeds.
Part 1: the views of the first 2000 frames of BASELINE cfg3's trajectory (small grid, one kb4 camera, up to 190 corners per view; the input of
tools/seed_timing.py) at the command line's defaults (principal point at the image centre, radius half of the half diagonal).  Device: the two
kernels of vc_seed_focal_batch alone (vc_time_seed_focal_batch: HIP events, runs back to back) and the whole call (allocation, uploads, kernels,
read-back: a host clock around it, best of 3 after one call that warms up).  Host: the one-lane build of the same arithmetic
(tests/host_harness/seed_focal_harness.cpp) on the same input, one thread, best of 3.
Part 2: the solve from the reference's start (fx = fy = 300, principal point at the centre, distortion 0) against the same start with fx = fy
seeded, poses from the device PnP with that camera in both, vision only: rows of the trace (vc_trace_len), cost of the first row, focal length
and RMSE at the end.  On the command-line test's dataset (poly3, 1280 x 960, f = 900, 40 frames) and on cfg3's kb4 camera.
Nothing is asserted: the figures go into DESIGN 4.16 and profiles/README.md.
   python tools/seed_focal_timing.py [n_frames]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from vicalib_amd import synth
from vicalib_amd.lib import ViCalibrator, seed_focal_batch, time_seed_focal_batch
import seed_focal_cases as sc


def arrays(p, frac=0.5):
    tiles = p.tiles
    off = np.concatenate([[0], np.cumsum([len(t[2]) for t in tiles])]).astype(np.int32)
    pw = np.concatenate([p.grid_points[t[2]] for t in tiles]); pc = np.concatenate([t[3] for t in tiles])
    cam = np.array([t[1] for t in tiles], dtype=np.int32)
    nc = len(p.cam_model)
    pp = np.tile([p.cfg.width / 2.0, p.cfg.height / 2.0], (nc, 1))
    rad = np.full(nc, frac * 0.5 * np.hypot(p.cfg.width, p.cfg.height))
    return cam, pp, rad, off, pw, pc


n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
cfg = synth.BASELINE_CONFIGS["cfg3"]
p3 = synth.generate(synth.Config(models=("kb4",), grid=cfg.grid, n_frames=n, imu=True))
a = arrays(p3)
print("cfg3: %d views, %d corners (%d .. %d per view)" % (len(a[0]), len(a[4]), np.diff(a[3]).min(), np.diff(a[3]).max()))
res = seed_focal_batch(*a)
wall = []
for _ in range(3):
    t0 = time.time(); seed_focal_batch(*a); wall.append(time.time() - t0)
ms = time_seed_focal_batch(*a, reps=10)
g = dict(views=[dict(cam=0, pw=p3.grid_points[t[2]], uv=t[3]) for t in p3.tiles], pp=a[1], radius=a[2], min_corners=4, max_fit_px=0.0)
host = []
sc.host_run(g)
for _ in range(3):
    t0 = time.time(); hres = sc.host_run(g); host.append(time.time() - t0)
print("kernels %.3f ms (%.2f us per view); whole call %.1f ms; one-lane host build %.1f ms; view status %s; f %.2f (true %.2f), host build %.2f"
      % (ms, 1e3 * ms / len(a[0]), 1e3 * min(wall), 1e3 * min(host), np.bincount(res["view_status"], minlength=5).tolist(), res["cam_f"][0], p3.cam_K_gt[0][0],
         hres["cam_f"][0]))


def solve(p, f):
    cal = ViCalibrator(0)
    for c, m in enumerate(p.cam_model):
        K = np.array(p.cam_K_init[c], dtype=np.float64)
        if f is not None:
            K[0] = K[1] = f[c]
        cal.AddCamera(m, K, p.cam_T_ck_init[c], p.cfg.width, p.cfg.height)
    for k in range(len(p.frame_time)):
        cal.AddFrame(np.array([0, 0, 0, 1.0, 0, 0, 1000.0]), p.frame_time[k])
    for (fr, c, ids, pix) in p.tiles:
        cal.AddObservations(fr, c, p.grid_points[ids], pix)
    cal.SetPnPDevice(True)
    seeded = cal.InitFramePosesPnP()
    cal.SetCalibrateImu(False)
    t0 = time.time()
    try:
        rc = cal.Solve()
    except Exception as e:
        rc = str(e)
    took = time.time() - t0
    tr = cal.trace()
    K, _ = cal.GetCamera(0)
    return dict(seeded=seeded, rc=rc, rows=len(tr), first=tr[0, 1] if len(tr) else float("nan"), last=tr[-1, 1] if len(tr) else float("nan"), f=K[0],
                rmse=cal.GetCameraProjRMSE()[0], secs=took)


cli = synth.generate(synth.Config(models=("poly3",), n_frames=40, seed=12, width=1280, height=960, gt_intrinsics=((900.0, 900.0, 645.0, 477.0, -0.28, 0.09, -0.012),)))
for label, p in (("poly3 1280 x 960, f = 900, 40 frames", cli), ("cfg3 kb4, %d frames, vision only" % n, p3)):
    r = seed_focal_batch(*arrays(p))
    print("%s: seed f %.2f (status %d, %d views); true %.2f" % (label, r["cam_f"][0], r["cam_status"][0], r["cam_views"][0], p.cam_K_gt[0][0]))
    for what, f in (("from 300", None), ("seeded", r["cam_f"] if r["cam_status"][0] == 0 else None)):
        s = solve(p, f)
        print("  %-9s %d frames with a pose seed; solve status %s; %d trace rows; cost of the first row %.6g, of the last %.6g; fx at the end %.3f; rmse %.4f px; %.2f s"
              % (what, s["seeded"], s["rc"], s["rows"], s["first"], s["last"], s["f"], s["rmse"], s["secs"]))
