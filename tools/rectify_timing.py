"""Time of the stereo consistency check (k_rectify_check) next to the two point inversions it contains.
The fov / fov stereo rig of BASELINE cfg2 (synthetic generator, ground-truth cameras, 0.1 px noise): its 500 frames' matched corners (about
95 k pairs), and the same pairs 100 times over as 50 000 frames (about 9.5 M pairs).  Device: Rectifier.time() (HIP events on the handle's
stream, 20 launches back to back after a warm-up, device-resident data).  Next to it, in the same process and alternating with it, side a's
Undistorter.time(): 65536 point inversions per launch, scaled to the check's 2 n inversions.  Writes profiles/rectify_timing.txt.
   python tools/rectify_timing.py [reps] [rounds] [output file]"""
import os, sys; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from vicalib_amd import synth
from vicalib_amd.lib import Rectifier

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

prob = synth.generate(synth.Config(models=("fov", "fov"), n_frames=500))
tf, tc, off, pw, pc = synth.flatten(prob)
ids = np.concatenate([t[2] for t in prob.tiles])
frames, foff, pa, pb = Rectifier.match_tiles(tf, tc, off, ids, 0, 1)
cams = [("fov", prob.cam_K_gt[c], (640, 480), prob.cam_T_ck_gt[c]) for c in (0, 1)]
lines = []
for copies in (1, 100):
    n1 = int(foff[-1])
    f_off = np.concatenate([[0], (np.diff(foff)[None, :].repeat(copies, 0).ravel()).cumsum()]).astype(np.int64)
    px_a, px_b, target = (np.tile(v, (copies, 1)) for v in (pc[pa], pc[pb], pw[pa]))
    r = Rectifier(cams[0], cams[1], dst_size=(640, 480), dst_linear=[300.0, 300.0, 319.5, 239.5])
    out = r.check(f_off, px_a, px_b, target)
    n = n1 * copies
    assert out["count"].sum() == n and not out["invalid"].any()
    check_ms, points_ms = [], []
    for _ in range(rounds):                       # alternating: both see the same clocks
        check_ms.append(r.time(reps))
        points_ms.append(r.side(0).time(n_images=1, reps=reps)["points"] * (2.0 * n / 65536.0))
    c, p = float(np.median(check_ms)), float(np.median(points_ms))
    lines.append("fov / fov, %d frames, %d pairs: check %.4f ms (%.1f Mpairs/s; rounds %s); the 2 n = %d point inversions alone, scaled from 65536 points: %.4f ms "
                 "(rounds %s); check / inversions %.2f; rms dv %.3f px, median rigid_rms %.3g m"
                 % (len(f_off) - 1, n, c, n / c / 1e3, " ".join("%.4f" % v for v in check_ms), 2 * n, p, " ".join("%.4f" % v for v in points_ms), c / p,
                    np.sqrt(out["sum_dv2"].sum() / n), np.median(out["rigid_rms"])))
    print(lines[-1], flush=True)
    r.close()
with open(sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "rectify_timing.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
