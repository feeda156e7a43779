"""The batches the predicted centre bias of a dot (vc_dot_bias_batch, vc_dot_bias.hpp) is held to, shared by tests/test_dot_bias_cpu.py (the host
build of its arithmetic, tests/host_harness/dot_bias_harness.cpp) and tests/test_dot_bias_gpu.py (the kernel).  The reference is
tests/dot_bias_ref.py, run once per group and kept.

A group is one batch: its views (model, intrinsics, T_cw, dot centres, radii).
  models   twelve views of the 9 x 6 board of tests/dot_images.py (30 mm pitch, radii 9.4 / 6.3 mm), one of every model twice, interleaved; tilts up
           to 0.6 rad at 0.35 to 0.55 m; 0, 1, 3, 40, 0, 64, 5, 65, 2, 0, 50 and 27 observations: 257 in all, views without any among them.  The
           batches of 0, 1, 3, 4, 5 and 257 observations are its prefixes (prefix()).
  axis     one view per model whose dot centre lies on the optical axis (the branch point of fov and kb4), tilted by 0.4 rad
  fronto   the whole board seen fronto-parallel by the linear camera, roll 0.3 rad: the bias is zero by symmetry
  sizes    linear, poly3 and kb4 views with r = 0, with dots of 2 px and of 40 px radius, and the linear view at 80 degrees of tilt
  status   a centre behind the camera (1), part of the rim behind the camera (2), a NaN pose (1), a dot so oblique and near that the
           estimate leaves it (4: |bias| / s is asserted to be above 1.2, away from the threshold), and a good dot between them

What is compared, and how (deviation()): status exactly; bias and radius_px by the largest absolute difference in pixels.  The bound is not
fixed in advance: the reference runs by two routes (the 5 x 5 normal equations, an SVD of the unsquared design), the spread between them is the
conditioning of a case, and the bound is 100 times the largest spread; bound() asserts that this is at most 1e-6 px.  It also asserts what the
groups promise: the statuses above, the reference within the bound of the exact ellipse centre (conic algebra) on every `linear` view, the
fronto-parallel biases below the bound, the radii of `sizes` in pixels."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import dot_bias_ref as ref
from vicalib_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODELS = ["fov", "poly2", "poly3", "kb4", "linear", "rational6"]
PARAMS = {"fov": [420.0, 418.0, 321.5, 238.0, 0.92], "poly2": [420.0, 421.0, 318.0, 241.0, -0.21, 0.06], "poly3": [415.0, 416.0, 322.0, 239.0, -0.28, 0.09, -0.012],
          "kb4": [260.0, 261.0, 319.0, 242.0, 0.012, -0.004, 0.0007, -0.0001], "linear": [420.0, 420.0, 319.5, 239.5],
          "rational6": [418.0, 419.0, 320.5, 240.5, 0.11, 0.021, 0.0012, 0.31, 0.034, 0.0021]}
GROUPS = ["models", "axis", "fronto", "sizes", "status"]
SIZES = [0, 1, 3, 40, 0, 64, 5, 65, 2, 0, 50, 27]
PREFIXES = [0, 1, 3, 4, 5, 257]
NX, NY, PITCH, R_LARGE, R_SMALL = 9, 6, 0.03, 0.0094, 0.0063
FILL = -7.0          # what the outputs hold before a run: a refused observation must leave it there


def board():
    """dot centres [54, 3] (board centred on the origin) and radii [54] of the board of tests/dot_images.py, pattern from a fixed seed"""
    ii, jj = np.meshgrid(np.arange(NX), np.arange(NY), indexing="xy")
    pw = np.stack([(ii.ravel() - 0.5 * (NX - 1)) * PITCH, (jj.ravel() - 0.5 * (NY - 1)) * PITCH, np.zeros(NX * NY)], axis=-1)
    big = np.random.default_rng(5).random(NX * NY) < 0.4
    return pw, np.where(big, R_LARGE, R_SMALL)


def pose(rotvec, t):
    return synth.se3_from_Rt(synth.so3_exp_matrix(np.asarray(rotvec, dtype=np.float64)), np.asarray(t, dtype=np.float64))


def _view(model, T_cw, pw, radius, params=None):
    return dict(model=model, params=np.asarray(PARAMS[model] if params is None else params, dtype=np.float64), T_cw=np.asarray(T_cw, dtype=np.float64),
                pw=np.ascontiguousarray(pw, dtype=np.float64).reshape(-1, 3), radius=np.ascontiguousarray(radius, dtype=np.float64).reshape(-1))


@functools.lru_cache(maxsize=None)
def group(name):
    pw, rad = board()
    rng = np.random.default_rng(17)
    if name == "models":
        views = []
        for k, n in enumerate(SIZES):
            axis = rng.standard_normal(3); axis[2] *= 0.3
            rot = axis / np.linalg.norm(axis) * rng.uniform(0.15, 0.6)
            T = pose(rot, [rng.uniform(-0.03, 0.03), rng.uniform(-0.02, 0.02), rng.uniform(0.35, 0.55)])
            pick = np.sort(rng.choice(4 * len(pw), size=n, replace=False)) % len(pw) if n > len(pw) else np.sort(rng.choice(len(pw), size=n, replace=False))
            views.append(_view(MODELS[k % 6], T, pw[pick], rad[pick]))
        return dict(views=views)
    if name == "axis":
        return dict(views=[_view(m, pose([0.4, 0.0, 0.0] if k % 2 else [0.0, -0.4, 0.1], [0.0, 0.0, 0.4]), np.zeros((1, 3)), [R_LARGE]) for k, m in enumerate(MODELS)])
    if name == "fronto":
        return dict(views=[_view("linear", pose([0.0, 0.0, 0.3], [0.01, -0.02, 0.42]), pw, rad)], fronto=True)
    if name == "sizes":
        views = []
        for m in ("linear", "poly3", "kb4"):
            f, z = PARAMS[m][0], 0.40
            T = pose([0.35, -0.3, 0.1], [0.01, 0.0, z])
            C = np.array([[0.0, 0.0, 0.0], [0.03, 0.0, 0.0], [0.0, 0.03, 0.0], [-0.03, -0.03, 0.0]])
            views.append(_view(m, T, C, [0.0, 2.0 * z / f, 40.0 * z / f, 2.0 * z / f]))
        views.append(_view("linear", pose([np.deg2rad(80.0), 0.0, 0.0], [0.0, 0.0, 0.45]), pw[::7], rad[::7]))
        return dict(views=views, radii_px=[0.0, 2.0, 40.0, 2.0])
    if name == "status":
        good = (np.array([0.03, 0.0, 0.0]), R_LARGE)
        r4 = 0.02
        views = [_view("linear", pose([0.3, 0.0, 0.0], [0.0, 0.0, -0.4]), [good[0], good[0]], [good[1], 0.0]),                     # behind the camera, also with r = 0
                 _view("poly3", pose([1.0, 0.0, 0.0], [0.0, 0.0, 0.1]), [np.zeros(3), good[0]], [0.2, good[1]]),                    # the rim crosses the camera's plane
                 _view("kb4", np.concatenate([[np.nan, 0.0, 0.0, 1.0], [0.0, 0.0, 0.4]]), [good[0]], [good[1]]),                    # a NaN pose
                 _view("linear", pose([1.0, 0.0, 0.0], [0.0, 0.0, r4 * np.sin(1.0) / 0.9]), [np.zeros(3)], [r4]),                    # the estimate leaves the dot
                 _view("fov", pose([0.2, 0.3, 0.0], [0.0, 0.0, 0.4]), [good[0]], [good[1]])]
        return dict(views=views, expect=[ref.NO_CENTRE, ref.NO_CENTRE, ref.NO_RIM, ref.OK, ref.NO_CENTRE, ref.LEFT_DOT, ref.OK])
    raise KeyError(name)


def batch_arrays(g, keep=None):
    """(models, params, T_cw, view_off, p_w, radius) of vicalib_amd.lib.dot_bias_batch; keep: the indices of the observations that go in (every
    view stays, with what is kept of it)"""
    views = g["views"]
    sizes = [len(v["radius"]) for v in views]
    first = np.concatenate([[0], np.cumsum(sizes)])
    sel = [np.arange(n) if keep is None else np.array([i - first[k] for i in keep if first[k] <= i < first[k + 1]], dtype=int) for k, n in enumerate(sizes)]
    off = np.concatenate([[0], np.cumsum([len(s) for s in sel])]).astype(np.int32)
    pw = np.concatenate([v["pw"][s] for v, s in zip(views, sel)]) if views else np.zeros((0, 3))
    rad = np.concatenate([v["radius"][s] for v, s in zip(views, sel)]) if views else np.zeros(0)
    T = np.array([v["T_cw"] for v in views]).reshape(-1, 7)
    return [v["model"] for v in views], [v["params"] for v in views], T, off, pw, rad


def prefilled(n):
    return dict(bias=np.full((n, 2), FILL), radius_px=np.full(n, FILL))


@functools.lru_cache(maxsize=None)
def reference(name, route="normal"):
    return ref.batch(*batch_arrays(group(name)), route=route)


def deviation(got, want, where="", rows=None):
    """the measures of the module's docstring, worst over the batch; asserts what has to agree exactly.  rows: the rows of `want` that `got` holds"""
    rows = np.arange(len(want["status"])) if rows is None else np.asarray(rows, dtype=int)
    assert np.array_equal(got["status"], want["status"][rows]), (where, got["status"], want["status"][rows])
    ok = want["status"][rows] == ref.OK
    worst = dict(bias=0.0, radius_px=0.0)
    if ok.any():
        worst["bias"] = float(np.abs(np.asarray(got["bias"])[ok] - want["bias"][rows][ok]).max())
        worst["radius_px"] = float(np.abs(np.asarray(got["radius_px"])[ok] - want["radius_px"][rows][ok]).max())
    assert np.isfinite(worst["bias"]) and np.isfinite(worst["radius_px"]), (where, worst)
    return worst


@functools.lru_cache(maxsize=None)
def bound():
    """(the bound in pixels, the spread of every group); asserts what the groups promise about the reference's output"""
    spreads = {}
    for name in GROUPS:
        spreads[name] = max(deviation(reference(name, "svd"), reference(name), name).values())
    b = 100.0 * max(spreads.values())
    assert 0.0 < b <= 1e-6, ("a case is too badly conditioned: replace it", spreads)
    for name in GROUPS:
        g, r = group(name), reference(name)
        if "expect" in g:
            assert r["status"].tolist() == g["expect"], (name, r["status"])
        else:
            assert (r["status"] == ref.OK).all(), (name, r["status"])
        i = 0
        for v in g["views"]:                                            # the exact ellipse centre where there is one
            m, K, R = synth.MODEL_IDS[v["model"]], np.zeros(10), synth.quat_to_matrix(v["T_cw"][:4])
            K[:len(v["params"])] = v["params"]
            for C, rr in zip(v["pw"], v["radius"]):
                if v["model"] == "linear" and r["status"][i] == ref.OK:
                    p0 = ref.project_jac(m, K, R @ C + v["T_cw"][4:])[0]
                    err = np.abs(p0 + r["bias"][i] - ref.linear_ellipse_centre(K, v["T_cw"], C, rr)).max() if rr > 0 else np.abs(r["bias"][i]).max()
                    assert err <= b, (name, i, "the reference against the exact ellipse centre", err, b)
                i += 1
        if g.get("fronto"):
            assert np.abs(r["bias"]).max() <= b, (name, np.abs(r["bias"]).max())
    sizes = reference("sizes")
    for k in range(3):
        got, want = sizes["radius_px"][4 * k:4 * k + 4], np.array(group("sizes")["radii_px"])
        assert np.all(np.abs(got - want) <= 0.15 * want + 1e-300), (k, got)          # (first order, tilted, off the axis: the nominal size to 15 %)
        assert np.all(sizes["bias"][4 * k] == 0.0) and sizes["radius_px"][4 * k] == 0.0
    v4 = group("status")["views"][3]
    K4 = np.zeros(10); K4[:4] = v4["params"]
    st, s, l = ref.lines(4, K4, v4["T_cw"], v4["pw"][0], v4["radius"][0])
    a, bb, c = l.T
    Kd = np.stack([a * a, a * bb, bb * bb, a * c, bb * c], axis=1)
    th = np.linalg.lstsq(Kd, -(c * c), rcond=None)[0]
    assert 0.5 * np.hypot(th[3], th[4]) > 1.2, ("the status-4 dot sits too close to the threshold", 0.5 * np.hypot(th[3], th[4]))
    assert reference("status")["status"][1] == ref.NO_CENTRE                        # (r = 0 does not rescue a centre behind the camera)
    return b, spreads


def check(name, got, label="", rows=None):
    """got: the dict of vicalib_amd.lib.dot_bias_batch, run on arrays prefilled with FILL.  Prints the worst value / bound."""
    b, _ = bound()
    want = reference(name)
    worst = deviation(got, want, name, rows)
    print("%s%s: bound %.3e px; worst of value / bound -- bias %.3e, radius_px %.3e" % (name, label, b, worst["bias"] / b, worst["radius_px"] / b))
    assert max(worst.values()) <= b, (name, worst, b)
    refused = got["status"] != ref.OK                                   # a refused observation: the caller's values are still there
    assert np.all(np.asarray(got["bias"])[refused] == FILL) and np.all(np.asarray(got["radius_px"])[refused] == FILL), name
    if group(name).get("fronto"):
        assert np.abs(got["bias"]).max() <= b, (name, np.abs(got["bias"]).max(), b)
    return worst


def prefix(n):
    """the first n observations of `models` (every view stays): (arrays, rows)"""
    rows = list(range(n))
    return batch_arrays(group("models"), keep=rows), rows


# ---------------------------------------------------------------------------------------------- the host build (tests/host_harness/dot_bias_harness.cpp)
def harness():
    src = os.path.join(HERE, "host_harness", "dot_bias_harness.cpp")
    so = os.path.join(HERE, "host_harness", "libvc_dot_bias_harness.so")
    deps = [src] + [os.path.join(ROOT, "vicalib_amd", "csrc", f) for f in ("vc_dot_bias.hpp", "vc_conic5.hpp", "vc_seed.hpp", "vc_undistort.hpp", "vc_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def c_arrays(models, params, T, off, pw, rad):
    """the arrays of the C ABI (padded where empty): model ids, K [n, 10], T, off, pw, rad"""
    m = np.array([synth.MODEL_IDS[x] for x in models], dtype=np.int32)
    K = np.zeros((len(models), 10))
    for v, p in enumerate(params):
        K[v, :len(p)] = p
    pad = lambda a, shape, dt: np.ascontiguousarray(a, dtype=dt) if len(a) else np.zeros(shape, dtype=dt)
    return pad(m, 1, np.int32), pad(K, (1, 10), np.float64), pad(T, (1, 7), np.float64), np.ascontiguousarray(off, dtype=np.int32), pad(pw, (1, 3), np.float64), pad(rad, 1, np.float64)


def host_run(arrays):
    """the host build on the batch, in the layout of vicalib_amd.lib.dot_bias_batch, on prefilled outputs"""
    n_views, n = len(arrays[0]), len(arrays[5])
    m, K, T, off, pw, rad = c_arrays(*arrays)
    out = prefilled(max(n, 1))
    status = np.full(max(n, 1), -1, dtype=np.int32)
    harness().dot_bias_harness_batch(n_views, _p(m), _p(K), _p(T), _p(off), _p(pw), _p(rad), _p(out["bias"]), _p(out["radius_px"]), _p(status))
    return dict(bias=out["bias"][:n], radius_px=out["radius_px"][:n], status=status[:n])


if __name__ == "__main__":
    b, spreads = bound()
    print("bound %.3e px; spreads %s" % (b, {k: "%.2e" % v for k, v in spreads.items()}))
    for name in GROUPS:
        check(name, host_run(batch_arrays(group(name))), label=" (host build)")
