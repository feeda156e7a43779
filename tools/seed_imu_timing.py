"""Time of the inertial seed (vc_seed_imu*) at the shapes of two baseline configurations: cfg3 (2000 frames at 20 Hz, a 200 Hz log, lags
+-0.5 s at the sample interval: 201 lags) and cfg5 (50 000 frames, a 1 kHz log, +-1 s: 2001 lags, 1e8 interval evaluations).  The motion is
the closed-form two-axis rotation of tests/seed_imu_cases.py with rotations at 0.1 degrees.
Device: the prefix integrals with the camera rates, the sweep with its finishing kernel, and the gravity sums, each set alone
(vc_time_seed_imu: HIP events, 10 runs back to back), and the whole call of vc_seed_imu -- upload, prefix integrals, coarse and fine sweep,
the picked lag, gravity, read-back -- by a host clock, best of 3 after one call that warms up.  Host: the one-thread build of the same
arithmetic (tests/host_harness/seed_imu_harness.cpp) on the same machine, the whole seed, once.  Nothing is asserted: the figures go into
DESIGN 4.19 and profiles/seed_imu_timing.txt.
   python tools/seed_imu_timing.py [cfg3|cfg5 ...]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import vicalib_amd.lib as lib
import seed_imu_cases as sc

SHAPES = {"cfg3": dict(n_int=1999, frame_rate=20.0, imu_rate=200.0, range_s=0.5), "cfg5": dict(n_int=49999, frame_rate=20.0, imu_rate=1000.0, range_s=1.0)}
FINE = 8

for name in (sys.argv[1:] or ["cfg3", "cfg5"]):
    s = SHAPES[name]
    p = sc.regular(s["n_int"], frame_rate=s["frame_rate"], imu_rate=s["imu_rate"], pad=s["range_s"] + 0.05, offset=0.12, seed=7)
    args = sc.DeviceSeedImu._args(p)
    step = 1.0 / s["imu_rate"]
    n_side = int(np.floor(s["range_s"] / step + 1e-9))
    lags = (np.arange(2 * n_side + 1) - n_side) * step
    print("%s: %d frames, %d samples, %d coarse lags + %d fine + 1: %.3e interval evaluations in the coarse sweep" %
          (name, len(p["frame_t"]), len(p["imu_t"]), len(lags), 4 * FINE + 1, len(lags) * s["n_int"]))

    def whole():
        t0 = time.time()
        r = lib.seed_imu(*args, range_s=s["range_s"], step_s=0.0, fine=FINE)
        return time.time() - t0, r

    whole()
    best, r = min((whole() for _ in range(3)), key=lambda x: x[0])
    ms = lib.time_seed_imu(*args, lags, reps=10)
    r2 = lib.seed_imu(*args, range_s=s["range_s"], step_s=0.0, fine=FINE)
    assert r["status"] == 0 and all(np.asarray(r[k]).tobytes() == np.asarray(r2[k]).tobytes() for k in r)
    print("device: prefix integrals and rates (4 launches) %.3f ms; coarse sweep (2 launches) %.3f ms = %.1f ps per interval evaluation; gravity %.3f ms"
          % (ms["prepare"], ms["sweep"], 1e9 * ms["sweep"] / (len(lags) * s["n_int"]), ms["gravity"]))
    print("device: whole call %.1f ms" % (1e3 * best))
    t0 = time.time(); h = sc.HostSeedImu.run(p, s["range_s"], 0.0, FINE); t1 = time.time()
    print("host, one thread: whole seed %.1f ms" % (1e3 * (t1 - t0)))
    e = sc.truth_errors(r, p["truth"])
    print("seed: offset %.6f s (error %.3g ms), rotation error %.3f degrees, bias error %.3g rad/s, gravity error %.3g rad, rms / signal %.4f, %d intervals"
          % (r["time_offset"], 1e3 * e["offset"], e["angle"], e["bias"], e["g_dir"], r["rms"] / r["signal"], r["count"]))
    print("device against the host build: offset %.3g s, rotation %.3g rad" % (abs(r["time_offset"] - h["time_offset"]), sc.ref.angle_between(r["R_ck"], h["R_ck"])))
