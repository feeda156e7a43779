"""Time of the camera-model conversion's kernels next to the comparer's fit sweep at the same lattice, from the same process.
Source: the generator's poly3 ground truth with the focal length scaled to the image's half-diagonal; targets kb4 (nk = 8, 47 sums per lane) and
rational6 (nk = 10, 68 sums per lane); lattices 64 x 48 on 640 x 480 and 2048 x 2048 on 2048 x 2048.  Device: Converter.time() (HIP events on the
handle's stream, launches back to back): the rays (one Newton inversion per sample), one linearisation (projection with the Jacobian with respect
to the intrinsics, J^T J packed), one cost sweep (one projection per sample), each with its one-wavefront reduction.  Beside it Comparer.time()[1],
the fit sweep (3 x 3 normal equations) of a comparer of the source against the result over the same fit set.  No threshold: the table states
what was measured.
   python tools/convert_timing.py [reps]      (writes profiles/convert_timing.txt)"""
import os, sys; ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np
from vicalib_amd import synth
from vicalib_amd.lib import Converter

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
lines = []
for (w, h), grid in (((640, 480), (64, 48)), ((2048, 2048), (2048, 2048))):
    K = np.array(synth.GT_INTRINSICS[synth.MODEL_IDS["poly3"]], dtype=np.float64)
    K[:2] *= np.hypot(w, h) / 800.0
    K[2:4] = (0.5 * w, 0.5 * h)
    for target in ("kb4", "rational6"):
        c = Converter(("poly3", K), target, (w, h), grid)
        out = c.run(1.0, 200)
        t = c.time(reps)
        cmp = c.comparer()
        fit = cmp.run(1.0)
        tc = cmp.time(reps)
        n = grid[0] * grid[1]
        lines.append("poly3 to %s, %d x %d lattice on %d x %d, %d samples in the fit set: rays %.4f ms; linearisation %.4f ms (%.1f Msamples/s); cost sweep %.4f ms "
                     "(%.1f Msamples/s); comparer's fit sweep over %d samples %.4f ms; linearisation / comparer's fit sweep %.2f; run: status %d after %d trials, "
                     "%.3g px rms, %.3g px max" % (target, grid[0], grid[1], w, h, out["n_fit"], t[0], t[1], out["n_fit"] / t[1] / 1e3, t[2], out["n_fit"] / t[2] / 1e3,
                                                    fit["n_fit"], tc[1], t[1] / tc[1], out["status"], out["iterations"],
                                                    np.sqrt(2.0 * out["cost"] / max(out["n_fit"], 1)), out["max_err"]))
        print(lines[-1], flush=True)
        cmp.close(); c.close()
with open(os.path.join(ROOT, "profiles", "convert_timing.txt"), "w") as f:
    f.write("tools/convert_timing.py, %d launches per figure (HIP events, back to back)\n" % reps + "\n".join(lines) + "\n")
