"""Time of the calibration comparison's kernels next to the point inversion they are built from.
kb4 and poly3 (the generator's ground-truth intrinsics, scaled with the image) against the same camera with the principal point moved by
(3, -2) px, a FULL lattice (one sample per pixel) at 640 x 480 and at 1280 x 960.  Device: Comparer.time() (HIP events on the handle's stream,
launches back to back): the rays (two Newton inversions per sample), one fit sweep (projection with Jacobian over the fit set), the difference
sweep (one projection per sample), each with its one-wavefront reduction.  Beside it Undistorter.time()'s 65536-point inversion on an
undistorter of the same camera and size, scaled to the 2 gx gy points the rays kernel inverts.  No threshold: the table states what was measured.
   python tools/compare_timing.py [reps]      (writes profiles/compare_timing.txt)"""
import os, sys; ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np
from vicalib_amd import synth
from vicalib_amd.lib import Comparer, Undistorter

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
lines = []
for (w, h) in ((640, 480), (1280, 960)):
    for model in ("kb4", "poly3"):
        K = np.array(synth.GT_INTRINSICS[synth.MODEL_IDS[model]], dtype=np.float64)
        K[:4] *= w / 640.0
        Kb = K.copy(); Kb[2:4] += (3.0, -2.0)
        c = Comparer((model, K), (model, Kb), (w, h), (w, h))
        fit = c.run(0.5)
        s = c.summary()
        t = c.time(reps)
        u = Undistorter(model, K, (w, h), Undistorter.fit_linear(model, K, (w, h), alpha=0.0))
        pts = u.time(n_images=1, reps=reps)["points"]
        n = w * h
        lines.append("%s %d x %d, %d samples: rays %.4f ms (%.1f Msamples/s); 65536-point inversion %.4f ms, scaled to %d points %.4f ms; rays / scaled inversion %.2f; "
                     "fit sweep %.4f ms over %d samples; difference sweep %.4f ms (%.1f Msamples/s); run: status %d after %d steps, %.4f px rms, %d invalid"
                     % (model, w, h, n, t[0], n / t[0] / 1e3, pts, 2 * n, pts * 2 * n / 65536, t[0] / (pts * 2 * n / 65536), t[1], fit["n_fit"], t[2], n / t[2] / 1e3,
                        fit["status"], fit["iterations"], np.sqrt(s["sum_sq"] / max(s["count"], 1)), s["invalid"]))
        print(lines[-1], flush=True)
        c.close(); u.close()
with open(os.path.join(ROOT, "profiles", "compare_timing.txt"), "w") as f:
    f.write("tools/compare_timing.py, %d launches per figure (HIP events, back to back)\n" % reps + "\n".join(lines) + "\n")
