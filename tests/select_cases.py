"""Cases and checks shared by tests/test_select_cpu.py (the host build of vc_select.hpp) and tests/test_select_gpu.py (the kernels, through the C
ABI): the smallest shapes at which the selection can still go wrong.

TOLERANCES.  None is a free constant; each is derived per case from the reference's own error (tests/select_ref.py), on the CPU:
  * "the code means what the definition says" (central-difference reference): the reference evaluated at the two steps H1 and H2; NUMERIC_FACTOR = 4
    x the largest difference of a scaled entry of I_f between the two is allowed on I_f, and 4 x the largest difference between the first-round
    gains computed from the two on the gains (the steps' disagreement propagated through the gains).  Found (before the factor) over the cases
    that use it: I_f 1.9e-10 (linear) ... 3.6e-9 (kb4), gains 3.3e-9 (stereo fov with a start set) ... 2.0e-6 (kb4).
  * device and host build against the analytic reference: the reference in float64 against itself in numpy.longdouble on that case, times MARGIN =
    16: the largest difference of a scaled entry of I_f, of a relative scale, of a gain of any candidate in any round along the long-double
    sequence; cum and total share one figure, the larger of theirs (total is the end of the cum series: cum_N = total).  Where the float64 value
    happens to lie closer to the long-double one than half a unit in its last place, half a unit is taken (_err): a float64 result cannot be
    asked to come closer than the format resolves -- the float64 reference's total of the 67-frame case is 5.6e-17 from the long-double one, 0.004
    units in the last place of 87.6.  Found (before the factor): I_f 1.3e-14 (rational6 x 4) ... 8.2e-12 (kb4), scale 5.0e-15 ... 3.8e-12, gains
    1.7e-12 (fixed intrinsics) ... 2.0e-7 (linear: its marginalised information is nearly singular, the prior carries the first rounds), cum and
    total 1.1e-12 ... 2.0e-7.  The float64 reference subtracts two slogdet; the code under test sums log(p'_k / p_k) over the pivots and is the more
    accurate of the two, which is why it uses a small part of what it gets.
`python tests/select_cases.py` prints the figures per case.
I_f is compared after the reference's scaling (entries of order one; the unscaled entries span focal lengths squared to distortion units)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import select_ref as ref
from vicalib_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
H1, H2 = 2e-5, 1e-5            # the two steps of the central-difference reference
NUMERIC_FACTOR = 4.0
MARGIN = 16.0                   # what the code under test gets of the analytic reference's own float64-against-long-double error
SEPARATION = 1000.0             # an exact-sequence case has the reference's best and second-best gains this many tolerances apart, in every round

GRID_W, GRID_H, PITCH = 19, 10, 0.254 / 18.0
K_FREE = ref.KFREE
ALL_FREE = ref.ROT | ref.TRANS | ref.KFREE


def grid_points():
    ii, jj = np.meshgrid(np.arange(GRID_W), np.arange(GRID_H), indexing="xy")
    return np.stack([(ii.ravel() - (GRID_W - 1) / 2) * PITCH, (jj.ravel() - (GRID_H - 1) / 2) * PITCH, np.zeros(GRID_W * GRID_H)], axis=1)


def pose(rng, dist=(0.22, 0.45), tilt=0.45, shift=0.04):
    """a rig pose T_wk that looks at the target (the plane z = 0, centred on the origin) from z < 0"""
    w = rng.uniform(-tilt, tilt, 3) * np.array([1.0, 1.0, 0.6])
    R = synth.so3_exp_matrix(w)
    centre = np.array([rng.uniform(-shift, shift), rng.uniform(-shift, shift), 0.0])
    t = centre - R @ np.array([0.0, 0.0, rng.uniform(*dist)])
    return synth.se3_from_Rt(R, t)


def camera(model, c=0, flags=K_FREE):
    K = list(synth.GT_INTRINSICS[synth.MODEL_IDS[model]])
    R = synth.so3_exp_matrix(np.array([0.01 * c, -0.02 * c, 0.015 * c]))
    return (model, K, synth.se3_from_Rt(R, np.array([-0.05 * c, 0.004 * c, 0.002 * c])), flags)


def rig(model, n, fix_intrinsics=False):
    k = 0 if fix_intrinsics else ref.KFREE
    return [camera(model, c, k if c == 0 else (ref.ROT | ref.TRANS | k)) for c in range(n)]


def subset(rng, n):
    return np.sort(rng.choice(GRID_W * GRID_H, size=n, replace=False)) if n < GRID_W * GRID_H else np.arange(GRID_W * GRID_H)


def make(name, cameras, n_frames, sizes, k, seed, start=(), prior=1e-6, one_camera_every=0, numeric=True, **pose_kw):
    rng = np.random.default_rng(seed)
    poses = np.stack([pose(rng, **pose_kw) for _ in range(n_frames)])
    tiles = []
    for f in range(n_frames):
        for c in range(len(cameras)):
            if one_camera_every and c > 0 and f % one_camera_every == 1:
                continue                                           # this frame is seen by camera 0 only
            tiles.append((f, c, subset(rng, sizes[(f + c) % len(sizes)])))
    return dict(name=name, cameras=cameras, poses=poses, tiles=tiles, points=grid_points(), k=k, start=tuple(start), prior=prior, numeric=numeric)


def mixed_67():
    """67 frames of poly3, mono: every view size, a frame of 3 corners (7), two identical frames (20 = 21), a frame with a corner behind the camera
    (30: one more target point one metre behind it).  k = 67 > usable."""
    c = make("poly3_67", [camera("poly3")], 67, (190, 4, 63, 64, 65, 190, 33), 67, seed=11)
    t = {f: ids for f, _, ids in c["tiles"]}
    t[7] = t[7][:3]
    c["poses"][21] = c["poses"][20]; t[21] = t[20].copy()
    c["points"] = np.concatenate([c["points"], [[0.0, 0.0, -1.5]]])
    t[30] = np.concatenate([t[30], [GRID_W * GRID_H]])
    c["tiles"] = [(f, 0, t[f]) for f in range(67)]
    c["special"] = dict(three=7, twins=(20, 21), behind=30)
    return c


def claim_recording():
    """60 frames of poly3, mono: 50 near-duplicate fronto-parallel views from 0.45 m and, at every sixth position + 3 (never one the every-6th subsample
    takes), 10 tilted and close ones."""
    rng = np.random.default_rng(5)
    poses = []
    for f in range(60):
        if f % 6 == 3:
            poses.append(pose(rng, dist=(0.18, 0.24), tilt=0.6, shift=0.05))
        else:
            poses.append(pose(rng, dist=(0.449, 0.451), tilt=0.004, shift=0.001))
    tiles = [(f, 0, np.arange(GRID_W * GRID_H)) for f in range(60)]
    return dict(name="claim_poly3_60", cameras=[camera("poly3")], poses=np.stack(poses), tiles=tiles, points=grid_points(), k=10, start=(), prior=1e-6, numeric=False)


@functools.lru_cache(maxsize=None)
def cases():
    out = [make("mono_" + m, [camera(m)], 5, (190, 64, 65, 63, 190), 3, seed=20 + i) for i, m in enumerate(("fov", "poly2", "poly3", "kb4", "linear", "rational6"))]
    out.append(make("one_frame", [camera("poly2")], 1, (190,), 1, seed=3))
    out.append(mixed_67())
    out.append(make("fov_300", [camera("fov")], 300, (190, 64, 65, 63, 4, 33), 4, seed=13, numeric=False))
    out.append(make("stereo_fov", rig("fov", 2), 12, (190, 65, 64), 4, seed=14, one_camera_every=3))
    out.append(make("stereo_fov_start", rig("fov", 2), 12, (190, 65, 64), 3, seed=14, one_camera_every=3, start=(2, 9)))
    out.append(make("kb4_x3", rig("kb4", 3), 8, (190, 63), 3, seed=15))
    out.append(make("rational6_x4", rig("rational6", 4), 8, (190,), 3, seed=16, numeric=False))
    out.append(make("stereo_fixed_intrinsics", rig("poly3", 2, fix_intrinsics=True), 6, (190, 64), 6, seed=17))
    out.append(make("k_equals_n", [camera("poly3")], 5, (190,), 5, seed=18))
    out.append(claim_recording())
    return {c["name"]: c for c in out}


NAMES = ["mono_fov", "mono_poly2", "mono_poly3", "mono_kb4", "mono_linear", "mono_rational6", "one_frame", "poly3_67", "fov_300", "stereo_fov", "stereo_fov_start", "kb4_x3",
         "rational6_x4", "stereo_fixed_intrinsics", "k_equals_n", "claim_poly3_60"]
UNSUPPORTED = "rational6_x5"    # D = 74


def unsupported_case():
    return make(UNSUPPORTED, rig("rational6", 5), 2, (190,), 1, seed=19)


def flat(case):
    """the arrays of vc_select_add_tiles / the harness"""
    tf = np.array([t[0] for t in case["tiles"]], dtype=np.int32); tc = np.array([t[1] for t in case["tiles"]], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum([len(t[2]) for t in case["tiles"]])]).astype(np.int64)
    pid = np.concatenate([np.asarray(t[2]) for t in case["tiles"]]).astype(np.int32) if case["tiles"] else np.zeros(0, dtype=np.int32)
    return tf, tc, off, pid


# ---------------------------------------------------------------------------------------------- the reference of a case, computed once
@functools.lru_cache(maxsize=None)
def analytic(name, long_double=False):
    """scaled information, status and scale of a case by the analytic reference"""
    c = cases()[name]
    dt = np.longdouble if long_double else np.float64
    I, status, corners, behind = ref.frame_information(c, lambda cs, f, cam, ids: ref.analytic_rows(cs, f, cam, ids, dt), dt)
    s = ref.scaling(I, status)
    return dict(I=I, It=ref.scaled(I, s), scale=s, status=status, corners=corners, behind=behind)


@functools.lru_cache(maxsize=None)
def numeric(name, h):
    c = cases()[name]
    I, status, corners, behind = ref.frame_information(c, lambda cs, f, cam, ids: ref.numeric_rows(cs, f, cam, ids, h))
    return dict(I=I, status=status)


@functools.lru_cache(maxsize=None)
def selection(name, long_double=False):
    """the reference's selection of a case; the float64 one follows the long-double sequence, so that the two differ by rounding alone"""
    c = cases()[name]
    a = analytic(name, long_double)
    seq = None if long_double else selection(name, True)["order"]
    return ref.greedy(a["It"], a["status"], c["k"], c["start"], c["prior"], sequence=seq)


def _err(x64, xld):
    """the float64 reference's error against its long-double evaluation, the largest over the entries; where the float64 value happens to have rounded
    closer than half a unit in its last place, half a unit: no float64 result can be expected to come closer than the format resolves"""
    x64 = np.asarray(x64, dtype=np.longdouble); xld = np.asarray(xld, dtype=np.longdouble)
    if x64.size == 0:
        return 0.0
    half_ulp = np.spacing(np.abs(xld).astype(np.float64)).astype(np.longdouble) / 2
    return float(np.maximum(np.abs(x64 - xld), half_ulp).max())


@functools.lru_cache(maxsize=None)
def tolerances(name):
    """MARGIN x the analytic reference's float64-against-long-double error on this case: dict(I, scale, gain, cum, total)"""
    a, b = analytic(name), analytic(name, True)
    s, t = selection(name), selection(name, True)
    sb = b["scale"]
    eI = _err(ref.scaled(a["I"].astype(np.longdouble), sb), b["It"])
    es = _err(a["scale"] / sb, np.ones_like(sb))
    eg = max([_err(x[y >= 0], y[y >= 0]) for x, y in zip(s["rounds"], t["rounds"]) if (y >= 0).any()] + [0.0])
    ec = _err(s["cum"], t["cum"]) if len(t["cum"]) else 0.0
    et = _err(np.array([s["total"]]), np.array([t["total"]]))
    return dict(I=MARGIN * eI, scale=MARGIN * es, gain=MARGIN * eg, cum=MARGIN * max(ec, et), total=MARGIN * max(ec, et))


@functools.lru_cache(maxsize=None)
def numeric_tolerances(name):
    """NUMERIC_FACTOR x the central-difference reference's disagreement between its two steps: dict(I, gain)"""
    c = cases()[name]
    a, b = numeric(name, H1), numeric(name, H2)
    s = analytic(name)["scale"]
    Ia, Ib = ref.scaled(a["I"], s), ref.scaled(b["I"], s)
    S0 = ref.start_matrix(Ia, c["start"], c["prior"])
    ga = ref.gains_given(Ia, a["status"], S0, set(c["start"]))
    gb = ref.gains_given(Ib, b["status"], ref.start_matrix(Ib, c["start"], c["prior"]), set(c["start"]))
    return dict(I=NUMERIC_FACTOR * float(np.abs(Ia - Ib).max()), gain=NUMERIC_FACTOR * float(np.abs(ga - gb).max()), It=Ib, gains=gb)


def separation(name):
    """the smallest gap between the reference's best and second-best gain over the rounds, in units of the gain tolerance"""
    t = selection(name, True)
    tol = tolerances(name)["gain"]
    gaps = []
    for g, f in zip(t["rounds"], t["order"]):
        rest = np.delete(g, f)
        rest = rest[rest >= 0]
        if len(rest):
            gaps.append(float(g[f] - rest.max()))
    return (min(gaps) / tol) if gaps and tol > 0 else np.inf


# ---------------------------------------------------------------------------------------------- the host build (tests/host_harness/select_harness.cpp)
def harness():
    src = os.path.join(HERE, "host_harness", "select_harness.cpp")
    so = os.path.join(HERE, "host_harness", "libvc_select_harness.so")
    deps = [src] + [os.path.join(ROOT, "vicalib_amd", "csrc", f) for f in ("vc_select.hpp", "vc_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", so, src])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def rig_arrays(cameras):
    n = len(cameras)
    model = np.array([synth.MODEL_IDS[c[0]] for c in cameras], dtype=np.int32)
    params = np.zeros((n, 10))
    for i, c in enumerate(cameras):
        params[i, :len(c[1])] = c[1]
    T_ck = np.ascontiguousarray([c[2] for c in cameras], dtype=np.float64)
    flags = np.array([c[3] for c in cameras], dtype=np.int32)
    return model, params, T_ck, flags


def host_select(case, k=None, start=None, prior=None, threads=1):
    """the host build of a whole selection: (status, dict in the layout the checks take)"""
    model, params, T_ck, flags = rig_arrays(case["cameras"])
    tf, tc, off, pid = flat(case)
    poses = np.ascontiguousarray(case["poses"], dtype=np.float64)
    pts = np.ascontiguousarray(case["points"], dtype=np.float64)
    N, D = len(poses), ref.dim(case["cameras"])
    st = np.array(case["start"] if start is None else start, dtype=np.int32)
    Dn, n = C.c_int(0), C.c_int(0)
    total = C.c_double(0)
    fstat = np.zeros((N, 3), dtype=np.int32); info = np.zeros((N, min(D, 64), min(D, 64))); scale = np.zeros(min(D, 64))
    order = np.zeros(N, dtype=np.int32); gain = np.zeros(N); cum = np.zeros(N); last = np.zeros(N)
    rc = harness().vch_select(len(model), _p(model), _p(params), _p(T_ck), _p(flags), N, _p(poses), len(tf), _p(tf), _p(tc), _p(off), _p(pts), _p(pid),
                               int(case["k"] if k is None else k), _p(st), len(st), C.c_double(case["prior"] if prior is None else prior), int(threads),
                               C.byref(Dn), _p(fstat), _p(info), _p(scale), C.byref(n), _p(order), _p(gain), _p(cum), C.byref(total), _p(last))
    assert Dn.value == D
    if rc != 0:
        return rc, None
    m = n.value
    return 0, dict(I=info, scale=scale, status=fstat[:, 0].copy(), corners=fstat[:, 1].copy(), behind=fstat[:, 2].copy(), order=order[:m].copy(), gain=gain[:m].copy(),
                   cum=cum[:m].copy(), total=total.value, last_gains=last)


# ---------------------------------------------------------------------------------------------- the checks, for any implementation
def check_information(name, got):
    """got: dict(I [N, D, D] unscaled, scale, status, corners, behind) of the code under test"""
    a, tol = analytic(name), tolerances(name)
    assert np.array_equal(got["status"], a["status"]), (got["status"], a["status"])
    assert np.array_equal(got["corners"], a["corners"]) and np.array_equal(got["behind"], a["behind"])
    err = float(np.abs(ref.scaled(got["I"], a["scale"]) - a["It"]).max())
    es = float(np.abs(got["scale"] / a["scale"] - 1).max())
    print(f"{name}: I_f err {err:.3e} (tol {tol['I']:.3e}), scale err {es:.3e} (tol {tol['scale']:.3e})")
    assert err <= tol["I"], (err, tol["I"])
    assert es <= tol["scale"], (es, tol["scale"])
    assert np.all(got["I"][a["status"] == 1] == 0.0)
    return err


def check_selection(name, got):
    """got: dict(order, gain, cum, total) of the code under test.  The pick rule stated so that near-ties cannot make it flaky: at every round, given
    the set the code has chosen so far, the reference recomputes all gains; the code's pick must be within the gain tolerance of the best, and the
    reported gain must match."""
    c, a, tol = cases()[name], analytic(name), tolerances(name)
    r = ref.greedy(a["It"], a["status"], c["k"], c["start"], c["prior"], sequence=got["order"])
    usable_left = int((a["status"] != 1).sum()) - len([f for f in c["start"] if a["status"][f] != 1])
    assert len(got["order"]) == len(r["order"]) == min(c["k"], usable_left), (len(got["order"]), len(r["order"]), usable_left)
    assert len(set(got["order"].tolist())) == len(got["order"]) and not set(got["order"].tolist()) & set(c["start"])
    worst = 0.0
    for k, f in enumerate(got["order"]):
        g = r["rounds"][k]
        assert g[f] >= 0, f"round {k}: frame {f} is not a candidate"
        assert g[f] >= g.max() - tol["gain"], (k, f, g[f], g.max())
        worst = max(worst, abs(got["gain"][k] - g[f]), abs(got["cum"][k] - r["cum"][k]))
        assert abs(got["gain"][k] - g[f]) <= tol["gain"], (k, got["gain"][k], g[f])
        assert abs(got["cum"][k] - r["cum"][k]) <= tol["cum"], (k, got["cum"][k], r["cum"][k])
    print(f"{name}: gain / cum err {worst:.3e} (tol {tol['gain']:.3e} / {tol['cum']:.3e}), total err {abs(got['total'] - r['total']):.3e} (tol {tol['total']:.3e})")
    assert abs(got["total"] - r["total"]) <= tol["total"], (got["total"], r["total"])
    return r


if __name__ == "__main__":
    for n in NAMES:
        t = tolerances(n)
        line = f"{n:26s} D {ref.dim(cases()[n]['cameras']):3d}  I {t['I'] / MARGIN:.2e} scale {t['scale'] / MARGIN:.2e} gain {t['gain'] / MARGIN:.2e} cum {t['cum'] / MARGIN:.2e} " \
               f"total {t['total'] / MARGIN:.2e}  separation {separation(n):.3g}"
        if cases()[n]["numeric"]:
            u = numeric_tolerances(n)
            line += f"  numeric I {u['I'] / NUMERIC_FACTOR:.2e} gain {u['gain'] / NUMERIC_FACTOR:.2e}"
        print(line)
