"""Time of greedy view selection on the device next to the host build of the same selection.
The 2000 frames of BASELINE cfg3's trajectory (small grid, up to 190 corners per view) at K = 200, cameras and poses at ground truth: once as the kb4
mono camera (intrinsics free, D = 8) and once as a stereo fov rig (camera 1 fully free, D = 16).  Device: Selector.time() (HIP events, launches back
to back: the information sweep, one gain round over every candidate left, one pick) and a complete Selector.run (upload, information sweep, K rounds,
one copy back; host clock around the synchronising call, median of five).  Host: tests/host_harness/select_harness.cpp, the same arithmetic
compiled with g++ -O2, on 16 threads, through its Python wrapper (median of three).
   python tools/select_timing.py [n_frames] [k]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from vicalib_amd import synth
from vicalib_amd.lib import Selector, CAM_ROT_FREE, CAM_TRANS_FREE, CAM_K_FREE
import select_cases as sc

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
k = int(sys.argv[2]) if len(sys.argv) > 2 else 200
names = {v: m for m, v in synth.MODEL_IDS.items() if m in ("fov", "poly2", "poly3", "kb4", "linear", "rational6")}
for models in (("kb4",), ("fov", "fov")):
    cfg = synth.BASELINE_CONFIGS["cfg3"]
    p = synth.generate(synth.Config(models=models, grid=cfg.grid, n_frames=n, imu=True))
    cams = [(names[p.cam_model[c]], list(p.cam_K_gt[c]), p.cam_T_ck_gt[c], CAM_K_FREE if c == 0 else CAM_ROT_FREE | CAM_TRANS_FREE | CAM_K_FREE) for c in range(len(models))]
    case = dict(cameras=cams, poses=p.frame_T_wk_gt, tiles=[(t[0], t[1], t[2]) for t in p.tiles], points=p.grid_points, k=k, start=(), prior=1e-6)
    tf, tc, off, pid = sc.flat(case)
    s = Selector(cams)
    s.set_poses(case["poses"]); s.add_tiles(tf, tc, off, case["points"], pid)
    r = s.run(k)                                     # allocates, uploads, sweeps
    again, whole = [], []
    for rep in range(5):                             # medians of five
        t0 = time.time(); s.run(k); again.append(time.time() - t0)      # the rounds alone: the information is kept while the input stands
        s.set_poses(case["poses"])                                       # the same input again: upload and information sweep are repeated
        t0 = time.time(); s.run(k); whole.append(time.time() - t0)
    again, whole = float(np.median(again)), float(np.median(whole))
    ms = s.time(20)
    st = np.bincount(s.frames()["status"], minlength=3)
    label = "+".join(models)
    print("%s, D = %d, %d frames, %d corners, K = %d: information sweep %.3f ms, one gain round %.4f ms, one pick %.4f ms per launch; complete run %.1f ms "
          "(%.1f ms with the information kept); picked %d, status %s, share of the first 10 / 50 views %.4f / %.4f"
          % (label, s.D, n, len(pid), k, ms[0], ms[1], ms[2], 1e3 * whole, 1e3 * again, len(r["order"]), st.tolist(),
             r["cum"][min(9, len(r["cum"]) - 1)] / r["total"], r["cum"][min(49, len(r["cum"]) - 1)] / r["total"]))
    sc.host_select(dict(case, k=1), threads=16)     # builds the harness
    host = []
    for rep in range(3):
        t0 = time.time(); rc, h = sc.host_select(case, threads=16); host.append(time.time() - t0)
    host = float(np.median(host))
    print("%s: host build of the same selection on 16 threads: %.1f ms; same order: %s" % (label, 1e3 * host, bool(rc == 0 and np.array_equal(h["order"], r["order"]))))
