"""Time of depth registration on the device next to the host build of the same work.
640 x 480 poly3 into 640 x 480 poly3 (nearest) and into 1280 x 720 rational6 (footprint), the generator's ground-truth intrinsics scaled with the
image, 0.1 m sideways and a few degrees apart, batch 8, kind Z, 1 mm units.  Device: Registrar.time() (HIP events on the handle's stream, launches
back to back): table build, clear + scatter + resolve of the 8 device-resident images, gather, 65536 points; and a complete Registrar.depth
(upload, launches, download; host clock around the synchronising call, median of five).  Host: tests/host_harness/register_harness.cpp, the same
arithmetic compiled with g++ -O2 on ONE thread (a sequential scatter), median of three; its output is compared with the device's.  The rate of
the 64-bit atomicMin is the number of key updates the scatter issues (counted by the host build) over the time of clear + scatter + resolve: a
lower bound, since that time also holds the clear and the resolve.
   python tools/register_timing.py [reps] [output file]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from vicalib_amd.lib import Registrar
import register_cases as rc

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "register_timing.txt")
N = 8
SRC = (640, 480)
lines = []


def surface(n, size):
    """the images vc_time_register registers: a slanted surface of 1000 .. 2499 counts"""
    w, h = size
    kk, jj, ii = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), indexing="ij")
    return (1000 + (3 * ii + 5 * jj + 11 * kk) % 1500).astype(np.uint16)


for label, model_d, size_d, splat in (("nearest", "poly3", (640, 480), 0), ("footprint", "rational6", (1280, 720), 1)):
    cam_s = ("poly3", rc.scaled_gt("poly3", SRC), SRC, rc.T_S)
    cam_d = (model_d, rc.scaled_gt(model_d, size_d), size_d, rc.T_D)
    args = dict(cam_s=cam_s, cam_d=cam_d, unit_src=0.001, unit_dst=0.001, kind=0, splat=splat)
    r = Registrar(**args)
    imgs = surface(N, SRC)
    depth, index, counters = r.depth(imgs)
    whole = []
    for rep in range(5):
        t0 = time.time(); r.depth(imgs); whole.append(time.time() - t0)
    whole = float(np.median(whole))
    t = r.time(n_images=N, reps=reps)
    h = rc.HostRegistrar(**args)
    landed = np.zeros(N, dtype=np.int64)
    host = []
    for rep in range(3):
        t0 = time.time(); hd, hi, hc = h.depth(imgs, landed); host.append(time.time() - t0)
    host = float(np.median(host))
    same = bool(np.array_equal(hd, depth) and np.array_equal(hi, index) and np.array_equal(hc, counters))
    atomics = int(landed.sum())
    lines.append("poly3 %d x %d into %s %d x %d, %s, batch %d: table build %.4f ms; clear + scatter + resolve %.4f ms (%.0f images/s); gather %.4f ms; 65536 points %.4f ms "
                 "= %.1f Mpoints/s; complete depth call with upload and download %.2f ms"
                 % (SRC[0], SRC[1], model_d, size_d[0], size_d[1], label, N, t["tables"], t["depth"], N / t["depth"] * 1e3, t["gather"], t["points"],
                    65536 / t["points"] / 1e3, 1e3 * whole))
    lines.append("   %d candidates, %d key updates (64-bit atomicMin), %d pixels filled: at least %.2f G atomics/s; host build of the depth test on one thread %.1f ms "
                 "(%.0f x the device's launches); same bytes as the device: %s"
                 % (int(counters[:, 6].sum()), atomics, int(counters[:, 7].sum()), atomics / t["depth"] / 1e6, 1e3 * host, 1e3 * host / t["depth"], same))
    r.close()
text = "\n".join(lines) + "\n"
sys.stdout.write(text)
with open(out_path, "w") as f:
    f.write(text)
