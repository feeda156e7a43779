"""Time of the depth calibration on the device next to the host build of the same work and to the registrar's work on the same batch.
640 x 480 poly3, the generator's ground-truth intrinsics, batch 8, kind Z, 1 mm units, bins 4 x 3, a board of 1.2 m x 0.9 m seen from 1 m.
Device: DepthCalibrator.time() (HIP events on the handle's stream, launches back to back): table build, accumulate + fold of the 8
device-resident images, apply; and a complete DepthCalibrator.add (upload, launches, download of the counters; host clock around the
synchronising call, median of five).  Host: tests/host_harness/depthcal_harness.cpp, the same arithmetic compiled with g++ -O2 on ONE
thread, median of three; its counters are compared with the device's.  In the same process: Registrar.time() of the same camera into
itself (nearest), its clear + scatter + resolve of a batch of 8.
   python tools/depthcal_timing.py [reps] [output file]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from vicalib_amd.lib import DepthCalibrator, Registrar
import depthcal_cases as dc
import register_cases as rc

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "depthcal_timing.txt")
N = 8
SRC = (640, 480)
cam = ("poly3", rc.scaled_gt("poly3", SRC), SRC, rc.T_S)
args = dict(cam=cam, rect=dc.RECT, bins=(4, 3), unit=0.001, kind=0, v_ref=1000.0, min_cos=0.5, max_dev=100.0)
d = DepthCalibrator(**args)
poses = np.stack([dc.board_pose(1.0 + 0.01 * k, (2.0 * k, -1.5 * k)) for k in range(N)])
y, rule = d.expected(poses)                                      # the images the calibration predicts, with a ripple of a few counts
kk, jj, ii = np.meshgrid(np.arange(N), np.arange(SRC[1]), np.arange(SRC[0]), indexing="ij")
imgs = np.where(np.isfinite(y), np.clip(np.rint(np.nan_to_num(y) + (3 * ii + 5 * jj + 11 * kk) % 9 - 4), 1, 65535), 1000).astype(np.uint16)
counters = d.add(imgs, poses)
whole = []
for rep in range(5):
    t0 = time.time(); d.add(imgs, poses); whole.append(time.time() - t0)
whole = float(np.median(whole))
t = d.time(n_images=N, reps=reps)
h = dc.HostDepthCal(**args)
host = []
for rep in range(3):
    t0 = time.time(); hc = h.add(imgs, poses); host.append(time.time() - t0)
host = float(np.median(host))
r = Registrar(cam, cam, 0.001, 0.001, 0, 0)
tr = r.time(n_images=N, reps=reps)
px = N * SRC[0] * SRC[1]
lines = ["poly3 %d x %d, bins 4 x 3, batch %d: table build %.4f ms; accumulate + fold %.4f ms (%.0f images/s, %.2f Gpixel/s); apply (bilinear) %.4f ms (%.2f Gpixel/s); "
         "complete add call with upload and download %.2f ms" % (SRC[0], SRC[1], N, t["tables"], t["accumulate"], N / t["accumulate"] * 1e3, px / t["accumulate"] / 1e6,
                                                                  t["apply"], px / t["apply"] / 1e6, 1e3 * whole),
         "   %d of %d pixels used; host build of the accumulation on one thread %.1f ms (%.0f x the device's launches); same counters as the device: %s"
         % (int(counters[:, 7].sum()), px, 1e3 * host, 1e3 * host / t["accumulate"], bool(np.array_equal(hc, counters))),
         "   the registrar on the same batch (poly3 %d x %d into itself, nearest): clear + scatter + resolve %.4f ms, table build %.4f ms: the accumulation takes %.2f x that"
         % (SRC[0], SRC[1], tr["depth"], tr["tables"], t["accumulate"] / tr["depth"])]
text = "\n".join(lines) + "\n"
sys.stdout.write(text)
with open(out_path, "w") as f:
    f.write(text)
