"""Time of the IMU noise characterisation (vc_allan*) on a log of n = 2^21 samples (2.9 hours at 200 Hz), six channels of white noise plus a
random walk, 20 averaging factors per decade up to 1/9 of the log (97 factors).
Device: the five launches of the means and prefix sums and the two of the sweep, each set alone (vc_time_allan: HIP events, 10 runs back to
back), and the whole call -- create (transpose on the host, upload, scan), run (sweep, read-back), destroy -- by a host clock, best of 3 after
one call that warms up.  Host: the one-thread build of the same arithmetic (tests/host_harness/allan_harness.cpp) on the same machine, prefix
sums and sweep apart, once.  Nothing is asserted: the figures go into DESIGN 4.18 and profiles/allan_timing.txt.
   python tools/allan_timing.py [log2_n]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from vicalib_amd.lib import AllanAnalyzer, allan_factors, allan_fit
import allan_cases as ac

log2n = int(sys.argv[1]) if len(sys.argv) > 1 else 21
n = 1 << log2n
tau0 = 0.005
r = np.random.default_rng(1)
gyro = 2e-3 * r.standard_normal((n, 3)) + 3e-4 * np.sqrt(tau0) * np.cumsum(r.standard_normal((n, 3)), axis=0)
accel = 2e-2 * r.standard_normal((n, 3)) + 3e-3 * np.sqrt(tau0) * np.cumsum(r.standard_normal((n, 3)), axis=0) + np.array([0.0, 0.0, 9.81])
t = tau0 * np.arange(n)
m, e = allan_factors(n, 20, 1.0 / 9.0)
terms = int(np.sum(n - 2 * m.astype(np.int64) + 1))
print("n = 2^%d = %d samples, %d factors (1 .. %d), %.3e terms per channel, six channels" % (log2n, n, len(m), m[-1], terms))


def whole():
    t0 = time.time()
    a = AllanAnalyzer(gyro, accel, t)
    t1 = time.time()
    avar, _ = a.run(m)
    t2 = time.time()
    a.close()
    return time.time() - t0, t1 - t0, t2 - t1, avar


whole()
best = min((whole() for _ in range(3)), key=lambda x: x[0])
a = AllanAnalyzer(gyro, accel, t)
ms = a.time(m, reps=10)
avar, _ = a.run(m)
a.close()
assert avar.tobytes() == best[3].tobytes()
bytes_read = 6 * terms * 3 * 8
print("device: scan (5 launches) %.3f ms; sweep (2 launches) %.3f ms = %.2f ns per 1000 terms, %.2f TB/s of prefix sums read (three per term, from cache)"
      % (ms["scan"], ms["sweep"], 1e9 * ms["sweep"] / (6 * terms), bytes_read / (1e-3 * ms["sweep"]) / 1e12))
print("device: whole call %.1f ms (create with upload and scan %.1f ms, run with read-back %.1f ms)" % (1e3 * best[0], 1e3 * best[1], 1e3 * best[2]))
t0 = time.time(); h = ac.HostAllan(gyro, accel, t); t1 = time.time(); host, _ = h.run(m); t2 = time.time()
print("host, one thread: prefix sums %.1f ms, sweep %.1f ms (%.2f s per channel)" % (1e3 * (t1 - t0), 1e3 * (t2 - t1), (t2 - t1) / 6))
print("device against the host build: largest relative difference of adev %.2e" % ac._rel(avar, host))
for c, name in ((0, "gx"), (3, "ax")):
    f = allan_fit(tau0 * m, avar[c], e)
    print("%s: N %.4e (true %.4e), K %.4e (true %.4e), B %.3e, mask %d, rms log %.3f" % (name, f["N"], (2e-3, 2e-2)[c // 3] * np.sqrt(tau0), f["K"], (3e-4, 3e-3)[c // 3], f["B"], f["mask"], f["rms_log"]))
