"""Cases and checks of the target step (vc_target_refine_batch), shared by tests/test_target_refine_cpu.py (the host build of vc_target_refine.hpp,
tests/host_harness/target_refine_harness.cpp) and tests/test_target_refine_gpu.py (the kernels, through the C ABI): the smallest shapes at which the
step can still go wrong.  The reference is tests/target_refine_ref.py, run once per case and kept.

A case: cameras, poses, tiles (frame, camera, point ids, measured pixels), `points` (the current target), `nominal`, lambda.  The measurements
are projections of a TRUE board = nominal + a quadratic bow of 1 mm, x printed 0.2 % too wide and an in-plane wave of 0.2 mm, plus 0.05 px of
noise from a fixed seed, so that costs and steps are far from zero.  Boards are grids cut to P points; 3P = 63, 66, 129 lie either side of a
panel of the dense factorisation (32) and of a wavefront (64).

  p4_n1_fixed .. p117_views   P = 4, 5, 21, 22, 43, 117; N = 1, 2, 5, 67; views of 3 (frame status 1), 4, 63, 64 and 65 corners; D = 0
  mono_<model>                the six models, P = 43, N = 5, intrinsics free
  stereo_fov                  two cameras, extrinsics of the second and both intrinsics free; most dots are seen by both cameras of a frame
  mixed                       a dot seen in one view only, a dot never seen, a dot only ever behind the camera (status 1 both: their rows of
                              `refined` are their rows of `points`, bit for bit) and the frame status 2 that goes with it
  collinear                   a nominal target on a line (gauge rank 6) with `points` off it
  similarity                  points != nominal by defects PLUS a similarity (rotation, scale, translation), which the step projects out
  exact                       exact measurements of the nominal target: d = 0
  rational6_x5                D = 74: refused

TOLERANCE.  Not fixed in advance (the rule of 4.20): the reference runs by its two routes, the spread between them is the conditioning of a case,
and the code under test gets 100 x the largest spread between them on that case: one relative number per case (bounds() says how it is formed),
applied to refined (largest absolute difference in metres), cost and predicted_decrease.  Where the two routes happen to agree closer than half a
unit in the last place, half a unit is taken, as in tests/select_cases.py.  Only the exact case, whose residuals are zero in both routes, takes its
bound from a one-unit move of the measured pixels instead.  Statuses, counts and the gauge rank must match exactly.
`python tests/target_refine_cases.py` prints the figures per case."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import select_cases as sc
import select_ref as sref
import target_refine_ref as ref
from vicalib_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FACTOR = 100.0
H1, H2 = 2e-5, 1e-5             # the two steps of the central-difference check of the Jacobians
FILL = -7.0                     # what `refined` holds before a run that must leave it untouched
LAMBDA = 1.0e4                  # sigma = 0.01 m
WIDTH = 0.24


def board(P):
    """P points of a grid about WIDTH metres wide, centred on the origin, in the plane z = 0"""
    nx = int(np.ceil(np.sqrt(1.5 * P)))
    ny = int(np.ceil(P / nx))
    ii, jj = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    pitch = WIDTH / max(nx - 1, 1)
    g = np.stack([(ii.ravel() - (nx - 1) / 2) * pitch, (jj.ravel() - (ny - 1) / 2) * pitch, np.zeros(nx * ny)], axis=1)
    return g[:P].copy()


def defects(nominal):
    x, y = nominal[:, 0], nominal[:, 1]
    return np.stack([0.002 * x + 2e-4 * np.sin(25.0 * y), 2e-4 * np.sin(20.0 * x), 1e-3 * ((x / 0.12) ** 2 + 0.5 * (y / 0.12) ** 2)], axis=1)


def measure(cameras, poses, true, f, c, ids, rng, noise=0.05):
    m, K, T_ck, _ = cameras[c]
    T = poses[f]
    Rwk, Rck = sref.quat_R(T, np.float64), sref.quat_R(T_ck, np.float64)
    pc = (true[ids] - T[4:7]) @ Rwk @ Rck.T + np.asarray(T_ck[4:7])
    with np.errstate(all="ignore"):
        z = synth.project(sref.model_id(m), np.asarray(K, dtype=np.float64), pc)
    return z + (rng.normal(0.0, noise, z.shape) if noise > 0 else 0.0)


def make(name, cameras, P, n_frames, sizes, seed, noise=0.05, offset=None, nominal=None, skip_second_camera_every=0, true=None):
    rng = np.random.default_rng(seed)
    nominal = board(P) if nominal is None else nominal
    points = nominal.copy() if offset is None else nominal + offset
    true = nominal + defects(nominal) if true is None else true
    poses = np.stack([sc.pose(rng, dist=(0.3, 0.5), tilt=0.5, shift=0.03) for _ in range(n_frames)])
    tiles = []
    for f in range(n_frames):
        for c in range(len(cameras)):
            if skip_second_camera_every and c > 0 and f % skip_second_camera_every == 1:
                continue
            n = min(sizes[(f + c) % len(sizes)], P)
            ids = np.sort(rng.choice(P, size=n, replace=False)) if n < P else np.arange(P)
            tiles.append((f, c, ids, measure(cameras, poses, true, f, c, ids, rng, noise)))
    return dict(name=name, cameras=cameras, poses=poses, tiles=tiles, points=points, nominal=nominal, lam=LAMBDA, true=true)


def mixed():
    """46 points: the board of 43, 43 = a dot in the plane seen by frame 2 only, 44 = a dot no tile names, 45 = a dot one metre and a half behind the
    cameras that frame 3 names (never usable).  Frame 3 has status 2."""
    nominal = np.concatenate([board(43), [[0.13, 0.1, 0.0], [-0.13, 0.1, 0.0], [0.0, 0.0, -1.5]]])
    true = nominal + np.concatenate([defects(nominal[:45]), np.zeros((1, 3))])
    c = make("mixed", [sc.camera("poly3")], 46, 5, (43,), seed=41, nominal=nominal, true=true)
    rng = np.random.default_rng(42)
    tiles = []
    for f, cam, ids, z in c["tiles"]:
        ids = np.arange(43)
        if f == 2:
            ids = np.concatenate([ids, [43]])
        if f == 3:
            ids = np.concatenate([ids[:20], [45], ids[20:]])
        z = measure(c["cameras"], c["poses"], true, f, cam, ids, rng)
        z[~np.isfinite(z)] = 0.0
        tiles.append((f, cam, ids, z))
    c["tiles"] = tiles
    c["points"] = nominal + np.array([[0.0, 0.0, 0.0]] * 44 + [[1e-3, -2e-3, 3e-3]] + [[0.0, 0.0, 0.0]])      # the never-seen dot carries an offset that must survive
    c["special"] = dict(one_view=43, never=44, behind=45, behind_frame=3)
    return c


def collinear():
    """nominal: 21 points on a line (the similarity's rotation about it vanishes: gauge rank 6); points: the 7 x 3 board"""
    grid = board(21)
    line = np.linspace(-0.12, 0.12, 21)[:, None] * (np.array([1.0, 0.5, 0.2]) / np.linalg.norm([1.0, 0.5, 0.2]))[None, :]
    return make("collinear", [sc.camera("linear")], 21, 6, (21,), seed=43, nominal=line, offset=grid - line, true=grid + defects(grid))


def similarity():
    nominal = board(43)
    R = synth.so3_exp_matrix(np.array([0.004, -0.006, 0.01]))
    moved = 1.003 * (nominal + 0.5 * defects(nominal)) @ R.T + np.array([1e-3, -5e-4, 2e-3])
    return make("similarity", [sc.camera("poly2")], 43, 6, (43, 30), seed=44, offset=moved - nominal)


@functools.lru_cache(maxsize=None)
def cases():
    fixed = lambda m: [sc.camera(m, 0, 0)]
    out = [make("p4_n1_fixed", fixed("linear"), 4, 1, (4,), seed=30),
           make("p5_n2_fixed", fixed("poly3"), 5, 2, (5, 4), seed=31),
           make("p21_n5", [sc.camera("linear")], 21, 5, (21, 15, 21, 9, 21), seed=32),
           make("p22_n5", [sc.camera("poly3")], 22, 5, (22, 16), seed=33),
           make("p21_n67", [sc.camera("kb4")], 21, 67, (21, 15, 4, 21, 10), seed=34),
           make("p117_views", [sc.camera("poly2")], 117, 5, (3, 4, 63, 64, 65), seed=35)]
    out += [make("mono_" + m, [sc.camera(m)], 43, 5, (43, 30, 43, 25, 43), seed=36 + i) for i, m in enumerate(("fov", "poly2", "poly3", "kb4", "linear", "rational6"))]
    out.append(make("stereo_fov", sc.rig("fov", 2), 43, 6, (43, 35, 40), seed=45, skip_second_camera_every=4))
    out += [mixed(), collinear(), similarity()]
    out.append(make("exact", [sc.camera("poly3")], 43, 5, (43, 30), seed=46, noise=0.0, true=board(43)))
    return {c["name"]: c for c in out}


NAMES = ["p4_n1_fixed", "p5_n2_fixed", "p21_n5", "p22_n5", "p21_n67", "p117_views", "mono_fov", "mono_poly2", "mono_poly3", "mono_kb4", "mono_linear", "mono_rational6",
         "stereo_fov", "mixed", "collinear", "similarity", "exact"]
COMPARED = [n for n in NAMES if n != "exact"]      # (the exact case has residuals of rounding size: its cost and decrease are noise, its d is held to the bound)
EXPECT_RANK = {"collinear": 6}


SIM_OMEGA, SIM_SCALE, SIM_SHIFT = np.array([5e-8, -1e-7, 1.5e-7]), 1e-7, np.array([5e-9, 1e-8, -5e-9])


def moved_by_small_similarity(name):
    """the case with a pure similarity of up to 2e-8 m added to `points` (rotation, scale and translation about the nominal centroid)"""
    case = dict(cases()[name])
    u = case["nominal"] - case["nominal"].mean(axis=0)
    case["points"] = case["points"] + np.cross(SIM_OMEGA, u) + SIM_SCALE * u + SIM_SHIFT
    return case


def similarity_bound(name):
    """how far `refined` may move when moved_by_small_similarity() moves `points`, on a case with a real step d: the step turns and grows with the
    board, by at most (|omega| + |scale|) max|d| -- twice that is allowed, for the change of the Jacobians along with it -- plus the case's bound
    on refined.  (The similarity itself is some 50 times larger: a step that did not project it out would miss by that.)"""
    return 2.0 * (np.linalg.norm(SIM_OMEGA) + SIM_SCALE) * float(np.abs(reference(name)["d"]).max()) + bounds(name)[0]["refined"]


def unsupported_case():
    return make("rational6_x5", sc.rig("rational6", 5), 21, 2, (21,), seed=47)


@functools.lru_cache(maxsize=None)
def reference(name, route="normal"):
    return ref.step(cases()[name], route)


def _spread(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.maximum(np.abs(a - b), np.spacing(np.abs(a)) / 2).max())


def nudged(name):
    """the case with every measured pixel moved to a neighbouring float64 (signs from a fixed seed): a measurement is known to half a unit in its last
    place (6e-14 px at 300 px), and so is the residual of any implementation that rounds the projection differently"""
    case = dict(cases()[name])
    rng = np.random.default_rng(7)
    case["tiles"] = [(f, c, ids, np.nextafter(z, np.where(rng.random(z.shape) < 0.5, -np.inf, np.inf))) for f, c, ids, z in case["tiles"]]
    return case


@functools.lru_cache(maxsize=None)
def bounds(name):
    """FACTOR x the largest spread between the reference's two routes on this case: dict(refined [m], cost, predicted_decrease), and the spreads.
    "The largest spread" is ONE number per case, so it is relative: the distance between the two routes over the size of the quantity -- refined
    over the largest entry of the step d, cost and predicted_decrease over themselves --, each at least half a unit in the last place (1.1e-16),
    the largest of the three; every quantity is then allowed FACTOR x that number x its size.  The exact case alone has no such number (both routes
    share residuals that are exactly zero: d = 0, cost = 0): its refined is held to FACTOR x what route (a) moves when every measured pixel moves
    by one unit in its last place (nudged), and its cost and predicted_decrease are not compared."""
    a, b = reference(name), reference(name, "lstsq")
    assert a["result_status"] == ref.OK and b["result_status"] == ref.OK, name
    if name == "exact":
        c = ref.step(nudged(name))
        spreads = {k: _spread(a[k], c[k]) for k in ("refined", "cost", "predicted_decrease")}
        return {k: FACTOR * v for k, v in spreads.items()}, spreads
    size = dict(refined=float(np.abs(a["d"]).max()), cost=float(a["cost"]), predicted_decrease=float(a["predicted_decrease"]))
    assert all(v > 0.0 for v in size.values()), (name, size)
    rel = {k: max(float(np.abs(np.asarray(a[k]) - np.asarray(b[k])).max()) / size[k], np.finfo(np.float64).eps / 2) for k in size}
    worst = max(rel.values())
    spreads = dict({k: worst * size[k] for k in size}, relative=worst, per_quantity=rel)
    return {k: FACTOR * worst * size[k] for k in size}, spreads


def flat(case):
    tf = np.array([t[0] for t in case["tiles"]], dtype=np.int32); tc = np.array([t[1] for t in case["tiles"]], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum([len(t[2]) for t in case["tiles"]])]).astype(np.int64)
    pid = np.concatenate([np.asarray(t[2]) for t in case["tiles"]]).astype(np.int32)
    z = np.ascontiguousarray(np.concatenate([np.asarray(t[3]).reshape(-1, 2) for t in case["tiles"]]), dtype=np.float64)
    return tf, tc, off, pid, z


def lib_args(case):
    """the arguments of vicalib_amd.lib.target_refine_batch"""
    tf, tc, off, pid, z = flat(case)
    return dict(cameras=case["cameras"], poses=case["poses"], tile_frame=tf, tile_cam=tc, tile_off=off, point_id=pid, p_c=z, points=case["points"], nominal=case["nominal"],
                lam=case["lam"])


# ---------------------------------------------------------------------------------------------- the host build (tests/host_harness/target_refine_harness.cpp)
def harness():
    src = os.path.join(HERE, "host_harness", "target_refine_harness.cpp")
    so = os.path.join(HERE, "host_harness", "libvc_target_refine_harness.so")
    deps = [src] + [os.path.join(ROOT, "vicalib_amd", "csrc", f) for f in ("vc_target_refine.hpp", "vc_select.hpp", "vc_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_step(case, fill=None):
    """the host build of a whole step: (status, dict in the layout of vicalib_amd.lib.target_refine_batch)"""
    model, params, T_ck, flags = sc.rig_arrays(case["cameras"])
    tf, tc, off, pid, z = flat(case)
    poses = np.ascontiguousarray(case["poses"], dtype=np.float64)
    pts = np.ascontiguousarray(case["points"], dtype=np.float64); nom = np.ascontiguousarray(case["nominal"], dtype=np.float64)
    N, P = len(poses), len(pts)
    refined = np.full((P, 3), FILL if fill is None else fill); pstat = np.full(P, -1, dtype=np.int32); pcor = np.zeros(P, dtype=np.int32)
    fstat = np.zeros((N, 3), dtype=np.int32)
    rank, status = C.c_int(-1), C.c_int(-1)
    cost, pred = C.c_double(FILL), C.c_double(FILL)
    rc = harness().vch_target_refine(len(model), _p(model), _p(params), _p(T_ck), _p(flags), N, _p(poses), len(tf), _p(tf), _p(tc), _p(off), _p(pid), _p(z), _p(pts), _p(nom), P,
                                     C.c_double(case["lam"]), _p(refined), _p(pstat), _p(pcor), _p(fstat), C.byref(rank), C.byref(status), C.byref(cost), C.byref(pred))
    if rc != 0:
        return rc, None
    return 0, dict(refined=refined, point_status=pstat, point_corners=pcor, frame_status=fstat[:, 0].copy(), corners=fstat[:, 1].copy(), behind=fstat[:, 2].copy(),
                   gauge_rank=rank.value, result_status=status.value, cost=cost.value, predicted_decrease=pred.value)


# ---------------------------------------------------------------------------------------------- the checks, for any implementation
def check(name, got, label=""):
    """got: the dict of vicalib_amd.lib.target_refine_batch.  Prints the worst value / bound per quantity."""
    case, want = cases()[name], reference(name)
    b, _ = bounds(name)
    for k in ("point_status", "point_corners", "frame_status", "corners", "behind"):
        assert np.array_equal(got[k], want[k]), (name, k, got[k], want[k])
    assert got["gauge_rank"] == want["gauge_rank"] == EXPECT_RANK.get(name, 7), (name, got["gauge_rank"], want["gauge_rank"])
    assert got["result_status"] == ref.OK, name
    dead = want["point_status"] == 1
    assert np.array_equal(np.asarray(got["refined"])[dead].view(np.uint64), np.asarray(case["points"], dtype=np.float64)[dead].view(np.uint64)), (name, "an unobserved row moved")
    err = dict(refined=float(np.abs(got["refined"] - want["refined"]).max()), cost=abs(got["cost"] - want["cost"]),
               predicted_decrease=abs(got["predicted_decrease"] - want["predicted_decrease"]))
    gauge = ref.gauge_residual(case, got["refined"], got["point_status"])
    print("%s%s: value / bound -- refined %.3e (bound %.3e m), cost %.3e (%.3e), predicted_decrease %.3e (%.3e), |Q^T (refined - nominal)| %.3e" % (
        name, label, err["refined"] / b["refined"], b["refined"], err["cost"] / b["cost"], b["cost"], err["predicted_decrease"] / b["predicted_decrease"],
        b["predicted_decrease"], gauge / b["refined"]))
    if name in COMPARED:
        for k in err:
            assert err[k] <= b[k], (name, k, err[k], b[k])
    else:
        assert err["refined"] <= b["refined"], (name, err["refined"], b["refined"])
    assert gauge <= b["refined"], (name, "Q^T (refined - nominal)", gauge, b["refined"])
    assert got["predicted_decrease"] >= 0.0, (name, got["predicted_decrease"])
    return err


if __name__ == "__main__":
    for n in NAMES:
        b, s = bounds(n)
        r = reference(n)
        print("%-16s D %2d  spread refined %.2e m  cost %.2e (of %.3e)  predicted_decrease %.2e (of %.3e)  |d| max %.2e m" % (
            n, sref.dim(cases()[n]["cameras"]), s["refined"], s["cost"], r["cost"], s["predicted_decrease"], r["predicted_decrease"], np.abs(r["d"]).max()))
