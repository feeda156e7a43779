"""Time of the rig seed (vc_seed_rig) for an 8-camera rig whose cameras all see every frame (28 pairs): 2000 frames (1.1e8 comparisons in the
vote) and 50 000 frames (7e10).  The poses are built directly, as tests/seed_rig_cases.py builds them (0.2 degrees / 1 mm of noise on every
view), vectorised.  Device: the three kernels each alone (vc_time_seed_rig: HIP events, launches back to back) and the whole call -- index
of shared frames, upload, three launches, read-back, tree -- by a host clock, best of 3 after one call that warms up.  Host: the one-thread
build of the same arithmetic (tests/host_harness/seed_rig_harness.cpp), at 2000 frames only.  Nothing is asserted beyond equal bits of two
calls: the figures go into DESIGN 4.21 and profiles/seed_rig_timing.txt.
   python tools/seed_rig_timing.py [2000 50000 ...]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import vicalib_amd.lib as lib
import seed_rig_cases as sc

C = 8


def qmul(a, b):
    return np.stack([a[..., 3] * b[..., 0] + a[..., 0] * b[..., 3] + a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 3] * b[..., 1] + a[..., 1] * b[..., 3] + a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 3] * b[..., 2] + a[..., 2] * b[..., 3] + a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0],
                     a[..., 3] * b[..., 3] - a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1] - a[..., 2] * b[..., 2]], axis=-1)


def qrot(q, v):
    u = 2.0 * np.cross(q[..., :3], v)
    return v + q[..., 3:4] * u + np.cross(q[..., :3], u)


def qexp(w):
    th = np.linalg.norm(w, axis=-1, keepdims=True)
    return np.concatenate([np.sin(0.5 * th) * w / np.maximum(th, 1e-300), np.cos(0.5 * th)], axis=-1)


def rig_views(n, seed=1):
    rng = np.random.default_rng(seed)
    q_c0 = qexp(np.deg2rad(15.0) * rng.uniform(-1, 1, size=(C, 3))); q_c0[0] = [0, 0, 0, 1]
    t_c0 = rng.uniform(-0.2, 0.2, size=(C, 3)); t_c0[0] = 0.0
    q_0w = qexp(np.deg2rad(30.0) * rng.uniform(-1, 1, size=(n, 3)))
    t_0w = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), rng.uniform(0.5, 1.0, n)], axis=-1)
    q = qmul(q_c0[None, :, :], q_0w[:, None, :]); t = qrot(q_c0[None, :, :], t_0w[:, None, :]) + t_c0[None, :, :]
    dq = qexp(np.deg2rad(0.2) * rng.normal(size=(n, C, 3)) / np.sqrt(3.0))
    T = np.concatenate([qmul(dq, q), qrot(dq, t) + rng.normal(scale=1e-3, size=(n, C, 3))], axis=-1)
    return np.ones((n, C), dtype=np.uint8), np.ascontiguousarray(T), np.concatenate([q_c0, t_c0], axis=-1)


for n in [int(a) for a in sys.argv[1:]] or [2000, 50000]:
    ok, T, truth = rig_views(n)
    print("%d frames x %d cameras: %d pairs, %.3e comparisons in the vote" % (n, C, C * (C - 1) // 2, C * (C - 1) // 2 * float(n) * n))

    def whole():
        t0 = time.time()
        r = lib.seed_rig(ok, T, tol_deg=3.0)
        return time.time() - t0, r

    whole()
    best, r = min((whole() for _ in range(3)), key=lambda x: x[0])
    r2 = lib.seed_rig(ok, T, tol_deg=3.0)
    assert (r["cam_status"] == 0).all() and all(r[k].tobytes() == r2[k].tobytes() for k in r)
    ms = lib.time_seed_rig(ok, T, tol_deg=3.0, reps=10 if n <= 4000 else 2)
    print("device: candidates %.3f ms, vote %.3f ms = %.2f ps per comparison, winner and refit %.3f ms; whole call %.1f ms"
          % (ms["candidates"], ms["support"], 1e9 * ms["support"] / (28.0 * n * n), ms["finish"], 1e3 * best))
    print("seed: support %d .. %d of %d, rms %.3f degrees %.2e m; worst camera %.4f degrees, %.2e m from the truth"
          % (r["pair_support"].min(), r["pair_support"].max(), n, r["pair_rms_deg"].max(), r["pair_rms_m"].max(),
             max(np.rad2deg(2 * np.arccos(min(1.0, abs(float(r["cam_T_c0"][c, :4] @ truth[c, :4]))))) for c in range(C)), np.abs(r["cam_T_c0"][:, 4:] - truth[:, 4:]).max()))
    if n <= 4000:
        t0 = time.time(); h = sc.host_seed_rig(ok, T, 3.0, 3); t1 = time.time()
        print("host, one thread: %.1f ms; device against it: %.2e on pair_T_ab, supports equal: %s"
              % (1e3 * (t1 - t0), np.abs(h["pair_T_ab"] - r["pair_T_ab"]).max(), bool((h["pair_support"] == r["pair_support"]).all())))
