"""Time of the projection-uncertainty map's kernels.  Camera: the generator's ground truth of each model with the focal length scaled to the
image's half-diagonal; covariance: a diagonal one of plausible sizes; lattices 53 x 41 on 640 x 480 and 2048 x 2048 on 2048 x 2048; fit radius 0.5.
Device: Uncertainty.time() (HIP events on the handle's stream, launches back to back): the rays (one Newton inversion per sample), the sweep of
G and C (one projection with both Jacobian blocks per sample of the fit set) and the map sweep (the same projection, J Cov J^T, summary and
rings), the last two with their one-wavefront reduction.  No threshold: the table states what was measured.
   python tools/uncertainty_timing.py [reps]      (writes profiles/uncertainty_timing.txt)"""
import os, sys; ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np
from vicalib_amd import synth
from vicalib_amd.lib import Uncertainty

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
lines = []
for (w, h), grid in (((640, 480), (53, 41)), ((2048, 2048), (2048, 2048))):
    for model in ("linear", "poly3", "kb4", "rational6"):
        K = np.array(synth.GT_INTRINSICS[synth.MODEL_IDS[model]], dtype=np.float64)
        K[:2] *= np.hypot(w, h) / 800.0
        K[2:4] = (0.5 * w, 0.5 * h)
        nk = len(K)
        cov = np.diag(np.array([0.3, 0.3, 0.5, 0.5] + [1e-3] * (nk - 4)) ** 2)
        u = Uncertainty((model, K), (w, h), grid)
        fit = u.run(cov, 1.0, 0.5)
        s = u.summary()
        t = u.time(reps)
        n = grid[0] * grid[1]
        lines.append("%s (nk %d), %d x %d lattice on %d x %d, %d samples, %d in the fit set: rays %.4f ms; Gram sweep %.4f ms; map sweep %.4f ms (%.1f Msamples/s); "
                     "worst sigma_max %.3g px, rms %.3g px" % (model, nk, grid[0], grid[1], w, h, n, fit["n_fit"], t[0], t[1], t[2], n / t[2] / 1e3,
                                                                np.sqrt(s["max_lam"]), np.sqrt(s["sum_var"] / max(s["count"], 1))))
        print(lines[-1], flush=True)
        u.close()
with open(os.path.join(ROOT, "profiles", "uncertainty_timing.txt"), "w") as f:
    f.write("tools/uncertainty_timing.py, %d launches per figure (HIP events, back to back)\n" % reps + "\n".join(lines) + "\n")
