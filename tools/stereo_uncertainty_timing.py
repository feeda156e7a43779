"""Time of the stereo uncertainty map's kernels.  Cameras: the generator's ground truth of each model with the focal length scaled to the image's
half-diagonal, the second 12 cm to the right of the first and turned by 5 degrees about y; destination camera: fitted at alpha 0; covariance: a
diagonal one of plausible sizes (1e-3 rad, 1e-3 m, 0.3 px, 0.5 px, 1e-3); lattices 53 x 41 on 640 x 480 and 1024 x 1024 on 2048 x 2048; depths
0.5, 2 and 5 m.  Device: StereoUncertainty.time() (HIP events on the handle's stream, launches back to back) on the last depth plane: the two side
sweeps (one projection with both Jacobian blocks per sample and side) and the map sweep (both blocks read, one pass over the packed 27 x 27
covariance in LDS, the triple, the summary) with its one-wavefront reduction.  No threshold: the table states what was measured.
   python tools/stereo_uncertainty_timing.py [reps]      (writes profiles/stereo_uncertainty_timing.txt)"""
import os, sys; ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np
from vicalib_amd import synth
from vicalib_amd.lib import StereoUncertainty

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
depths = (0.5, 2.0, 5.0)
Ta = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
Rb = synth.so3_exp_matrix(np.deg2rad(5.0) * np.array([0.0, 1.0, 0.0]))
Tb = synth.se3_from_Rt(Rb, Rb @ np.array([-0.12, 0.0, 0.0]))
lines = []
for (w, h), grid in (((640, 480), (53, 41)), ((2048, 2048), (1024, 1024))):
    for pair in (("linear", "linear"), ("fov", "fov"), ("kb4", "poly3"), ("rational6", "poly2")):
        cams = []
        for model in pair:
            K = np.array(synth.GT_INTRINSICS[synth.MODEL_IDS[model]], dtype=np.float64)
            K[:2] *= np.hypot(w, h) / 800.0
            K[2:4] = (0.5 * w, 0.5 * h)
            cams.append((model, K))
        side = lambda nk: [0.5e-3] * 4 + [1e-3] * 3 + [0.3, 0.3, 0.5, 0.5] + [1e-3] * (nk - 4)
        cov = np.diag(np.array(side(len(cams[0][1])) + side(len(cams[1][1]))) ** 2)
        u = StereoUncertainty(cams[0], cams[1], (w, h), (w, h), Ta, Tb, alpha=0.0, grid=grid)
        u.run(cov, 1.0, depths)
        s = u.summary(len(depths) - 1)
        t = u.time(reps)
        n = grid[0] * grid[1]
        lines.append("%s / %s, %d x %d lattice on %d x %d, %d samples, %d valid at %g m: side sweeps %.4f ms; map sweep %.4f ms (%.1f Msamples/s); "
                     "rms sigma_dv %.3g px, rms sigma_Z / Z %.3g" % (pair[0], pair[1], grid[0], grid[1], w, h, n, s["count"], depths[-1], t[0], t[1], n / t[1] / 1e3,
                                                                      np.sqrt(s["sum_var_dv"] / max(s["count"], 1)), np.sqrt(s["sum_var_z"] / max(s["count"], 1)) / depths[-1]))
        print(lines[-1], flush=True)
        u.close()
with open(os.path.join(ROOT, "profiles", "stereo_uncertainty_timing.txt"), "w") as f:
    f.write("tools/stereo_uncertainty_timing.py, %d launches per figure (HIP events, back to back)\n" % reps + "\n".join(lines) + "\n")
