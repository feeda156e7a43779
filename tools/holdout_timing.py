"""Time of the held-out scoring next to the host pose refinement it replaces.
500 held-out frames of up to 190 corners: the views of the first 500 frames of BASELINE cfg3's trajectory (small grid, one camera), once as
kb4 and once as poly3, cameras at ground truth.  Device: ViCalibrator.time_holdout() (HIP events, launches back to back; PnP seeds and seeds
1 cm off the truth).  Host: vc_pnp_planar (homography + LM refinement of the 6 pose parameters) of the same views on 16 threads.
   python tools/holdout_timing.py [n_frames]"""
import os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from concurrent.futures import ThreadPoolExecutor
import numpy as np
from vicalib_amd import synth
from vicalib_amd.lib import ViCalibrator, pnp_planar

n = int(sys.argv[1]) if len(sys.argv) > 1 else 500
for model in ("kb4", "poly3"):
    cfg = synth.BASELINE_CONFIGS["cfg3"]
    p = synth.generate(synth.Config(models=(model,), grid=cfg.grid, n_frames=n, imu=True))
    cal = ViCalibrator(0)
    cal.AddCamera(model, p.cam_K_gt[0], p.cam_T_ck_gt[0], p.cfg.width, p.cfg.height)
    tf = np.array([t[0] for t in p.tiles], dtype=np.int32); tc = np.array([t[1] for t in p.tiles], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum([len(t[2]) for t in p.tiles])]).astype(np.int64)
    cal.HoldoutAddTiles(tf, tc, off, p.grid_points, np.concatenate([t[2] for t in p.tiles]), np.concatenate([t[3] for t in p.tiles]))
    off_truth = p.frame_T_wk_gt.copy(); off_truth[:, 4] += 0.01
    for label, seeds in (("PnP seeds", None), ("seeds 1 cm off the truth", off_truth)):
        t0 = time.time(); res = cal.HoldoutCompute(seeds); wall = time.time() - t0
        ms = cal.time_holdout(20)
        st = np.bincount(res["frames"]["status"], minlength=5)
        print("%s, %d frames, %d corners, %s: pose refit %.3f ms, residual sweep %.4f ms per launch; iterations mean %.1f max %d; status %s; "
              "held-out RMSE %.4f px; whole compute (host seeds, uploads, both kernels, read-back) %.1f ms"
              % (model, len(res["frames"]["status"]), len(res["r"]), label, ms["pose"], ms["residuals"], res["frames"]["iterations"].mean(),
                 res["frames"]["iterations"].max(), st.tolist(), res["rmse"][0], 1e3 * wall))
    views = [(p.grid_points[t[2]], np.ascontiguousarray(t[3])) for t in p.tiles]
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(lambda v: pnp_planar(model, p.cam_K_gt[0], v[0], v[1]), views[:32]))
        t0 = time.time(); list(ex.map(lambda v: pnp_planar(model, p.cam_K_gt[0], v[0], v[1]), views)); host = time.time() - t0
    print("%s: host vc_pnp_planar of the same %d views on 16 threads: %.1f ms" % (model, len(views), 1e3 * host))
