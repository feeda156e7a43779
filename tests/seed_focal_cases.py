"""The batches the focal-length seed (vc_seed_focal_batch, vc_seed_focal.hpp) is held to, shared by tests/test_seed_focal_cpu.py (the host build of
its arithmetic, tests/host_harness/seed_focal_harness.cpp) and tests/test_seed_focal_gpu.py (the kernels).  The reference is
tests/seed_focal_ref.py, run once per group and kept.

A group is one batch: its views (camera, target points, pixels), the cameras' assumed principal points and radii, min_corners, max_fit_px.
  counts        one camera: views of 3 (refused), 4, 5, 8, 63, 64, 65 and 190 corners (the minimum; one corner per lane and one either side; a
                full board, three rounds per lane), a view with a NaN corner, a view with one target point off the plane
  models        six cameras, one of every model, three views each, interleaved frame by frame; radius half of 400 px
  radius        three cameras looking at the same view with radii that leave 3 (refused), 4 and all of its corners in
  fit_on / fit_off   a good view and one whose detections belong to the neighbouring dots, with max_fit_px = 1 px and without the test
  cams          four cameras, views interleaved: five tilted views, no view, three fronto-parallel views (noisy: their rows are small but
                well determined), one tilted view
  truth         two linear cameras (f = 400 and 520) seen exactly: no noise, the assumed principal point is the true one, all corners
  cap_fov / cap_poly3 / cap_kb4   40 views of one distorted camera at the generator's intrinsics, noise 0.1 px, radius a quarter of the half diagonal

What is compared, and how (deviation()):
  exactly       view_status, view_used, cam_status, cam_views, which view_f are NaN
  H             after the reference's scaling and a sign fix, the largest entry of the difference over the largest entry of the reference
  rows          as pairs: |(c1, c2) - ref| / |ref| and |(d1, d2) - ref| / |ref| (a single entry of a pair may be zero by geometry)
  fit_px        relative, with a floor of 0.01 px under the divisor: a fit of an exact view is rounding noise, and everything below a hundredth
                of a pixel is the same to max_fit_px and to the reader
  view_f, cam_f relative
The bound is not fixed in advance: the reference runs by two routes (eigh of the squared 9 x 9 matrix, svd of the unsquared DLT matrix), the
spread between them in the measures above is the conditioning of the case, and the bound is 100 times the largest spread (a Jacobi sweep on
the squared matrix in another summation order loses digits of the same order).  bound() asserts that this is not looser than 1e-6; a case
that makes it so is replaced.  It also asserts what the groups promise: the statuses above, the reference within 1e-8 of the true focal length
on `truth`, within 25 % on the three cap groups."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import seed_focal_ref as ref
from vicalib_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODELS = ["fov", "poly2", "poly3", "kb4", "linear", "rational6"]
COUNTS = [3, 4, 5, 8, 63, 64, 65, 190]
GROUPS = ["counts", "models", "radius", "fit_on", "fit_off", "cams", "truth", "cap_fov", "cap_poly3", "cap_kb4"]
PP = (320.0, 240.0)
FILL = -7.0          # what the outputs hold before a run: a refused view or camera must leave it there
MIN_TILT = 5.0


@functools.lru_cache(maxsize=None)
def _problem(models, seed, sigma, n_frames=60, K=None):
    return synth.generate(synth.Config(models=models, n_frames=n_frames, seed=seed, pixel_sigma=sigma, gt_intrinsics=K))


def _tiles(p, cam, at_least=4):
    return [t for t in p.tiles if t[1] == cam and len(t[2]) >= at_least]


def _take(p, tile, cam, n=None, seed=0):
    f, c, ids, pix = tile
    keep = np.arange(len(ids)) if n is None else np.sort(np.random.default_rng(1000 * seed + n).choice(len(ids), size=n, replace=False))
    return dict(cam=cam, pw=np.ascontiguousarray(p.grid_points[ids[keep]]), uv=np.ascontiguousarray(pix[keep]))


def _group(views, n_cams, radius, min_corners=4, max_fit_px=0.0, pp=None, **extra):
    pp = np.tile(np.array(PP), (n_cams, 1)) if pp is None else np.asarray(pp, dtype=np.float64)
    return dict(views=views, pp=pp, radius=np.broadcast_to(np.asarray(radius, dtype=np.float64), (n_cams,)).copy(), min_corners=min_corners, max_fit_px=max_fit_px,
                **extra)


def _fronto_view(cam, k):
    """the small grid seen by a linear camera (f = 400) whose image plane is parallel to it, 0.05 px noise: distance, shift and roll vary with k"""
    gw, gh, sp = synth.GRIDS["small"]
    ii, jj = np.meshgrid(np.arange(gw), np.arange(gh), indexing="ij")
    pw = np.stack([ii.ravel() * sp, jj.ravel() * sp, np.zeros(gw * gh)], axis=-1)
    a = 0.3 * k
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    pc = (pw - np.array([0.12 + 0.01 * k, 0.06, 0.0])) @ R.T + np.array([0, 0, 0.30 + 0.05 * k])
    uv = 400.0 * pc[:, :2] / pc[:, 2:3] + np.array(PP) + 0.05 * np.random.default_rng(77 + k).standard_normal((len(pw), 2))
    return dict(cam=cam, pw=pw, uv=np.ascontiguousarray(uv))


@functools.lru_cache(maxsize=None)
def group(name):
    if name == "counts":
        p = _problem(("linear",), 31, 0.05)
        views = []
        for k, n in enumerate(COUNTS):
            tiles = _tiles(p, 0, max(n, 4))
            assert tiles, n
            views.append(_take(p, tiles[(7 * k + 3) % len(tiles)], 0, n, seed=k))
        holed = _take(p, _tiles(p, 0, 64)[11], 0, 64, seed=91)
        holed["uv"][20, 1] = np.nan
        bent = _take(p, _tiles(p, 0, 64)[17], 0, 64, seed=92)
        bent["pw"][17, 2] += 0.05
        return _group(views + [holed, bent], 1, 0.0, expect=[ref.FEW] + [ref.OK] * 8 + [ref.NOT_PLANAR], expect_cam=[ref.CAM_OK])
    if name == "models":
        views = []
        for k in (2, 9, 16):                                     # (one problem per model: each camera sees the target from the same trajectory)
            for c, m in enumerate(MODELS):
                p = _problem((m,), 5 + c, 0.05)
                t = _tiles(p, 0, 100)
                views.append(_take(p, t[k % len(t)], c))
        return _group(views, 6, 200.0, expect_cam=[ref.CAM_OK] * 6)
    if name == "radius":
        p = _problem(("linear",), 31, 0.05)
        v = _take(p, _tiles(p, 0, 150)[5], 0)
        d = np.sort(np.linalg.norm(v["uv"] - np.array(PP), axis=1))
        assert d[2] + 0.5 < d[3] < d[4] - 0.5, "the radii need a gap between the third, fourth and fifth nearest corner: take another view"
        return _group([dict(v, cam=c) for c in range(3)], 3, [0.5 * (d[2] + d[3]), 0.5 * (d[3] + d[4]), 0.0], expect=[ref.FEW, ref.OK, ref.OK],
                      expect_used=[0, 4, len(d)])
    if name in ("fit_on", "fit_off"):
        p = _problem(("linear",), 31, 0.05)          # (a distorted lens does not fit a homography to 1 px over this radius)
        good =_take(p, _tiles(p, 0, 150)[3], 0)
        mixed = _take(p, _tiles(p, 0, 150)[9], 0)
        mixed["uv"] = np.ascontiguousarray(np.roll(mixed["uv"], 1, axis=0))            # every detection goes to the next dot
        return _group([good, mixed], 1, 200.0, max_fit_px=1.0 if name == "fit_on" else 0.0, expect=[ref.OK, ref.BAD_FIT if name == "fit_on" else ref.OK])
    if name == "cams":
        p = _problem(("linear",), 37, 0.05)
        t = _tiles(p, 0, 100)
        own = [_take(p, t[k], 0) for k in (2, 9, 16, 23, 30)]
        lone = _take(p, t[12], 3)
        flat = [_fronto_view(2, k) for k in range(3)]
        views = [own[0], flat[0], own[1], lone, flat[1], own[2], own[3], flat[2], own[4]]
        return _group(views, 4, 0.0, expect=[ref.OK] * 9, expect_cam=[ref.CAM_OK, ref.CAM_NO_VIEW, ref.CAM_NO_TILT, ref.CAM_OK])
    if name == "truth":
        K = ((400.0, 400.0) + PP, (520.0, 520.0) + PP)
        p = _problem(("linear", "linear"), 41, 0.0, K=K)
        views = [_take(p, t, t[1]) for t in p.tiles if t[0] in (4, 15, 26, 37, 48, 59)]
        return _group(views, 2, 0.0, expect_cam=[ref.CAM_OK] * 2, truth=[400.0, 520.0])
    if name.startswith("cap_"):
        model = name[4:]
        # Radius: a quarter of the half diagonal.  At half of it the reference misses the cap on this generator's fov (w = 0.92) and kb4
        # (f = 260 px at 640 x 480) cameras: 1.3 to 1.7 and 2.1 to 2.2 times the true focal length over the seeds 3, 7, 13; poly3 1.07 to
        # 1.29.  At a quarter: fov 1.04 to 1.19, poly3 0.97 to 1.10, kb4 0.95 to 1.13.  The seeds below are the best of the three.
        p = _problem((model,), {"fov": 3, "poly3": 3, "kb4": 13}[model], 0.1, n_frames=40)
        views = [_take(p, t, 0) for t in p.tiles]
        assert len(views) == 40
        return _group(views, 1, 0.25 * 0.5 * np.hypot(640.0, 480.0), expect_cam=[ref.CAM_OK], cap=float(p.cam_K_gt[0][0]))
    raise KeyError(name)


def batch_arrays(g, keep=None):
    """(view_cam, cam_pp, cam_radius, view_off, p_w, p_c) of vicalib_amd.lib.seed_focal_batch; keep: the indices of the views that go in"""
    views = g["views"] if keep is None else [g["views"][k] for k in keep]
    off = np.concatenate([[0], np.cumsum([len(v["pw"]) for v in views])]).astype(np.int32)
    pw = np.concatenate([v["pw"] for v in views]) if views else np.zeros((0, 3))
    uv = np.concatenate([v["uv"] for v in views]) if views else np.zeros((0, 2))
    return np.array([v["cam"] for v in views], dtype=np.int32), g["pp"], g["radius"], off, pw, uv


def prefilled(n, nc):
    return dict(view_H=np.full((n, 3, 3), FILL), view_rows=np.full((n, 4), FILL), view_f=np.full(n, FILL), view_fit_px=np.full(n, FILL),
                view_used=np.full(n, int(FILL), dtype=np.int32), cam_f=np.full(nc, FILL))


@functools.lru_cache(maxsize=None)
def reference(name, route="eigh"):
    g = group(name)
    return ref.batch(*batch_arrays(g), min_corners=g["min_corners"], max_fit_px=g["max_fit_px"], min_tilt_deg=MIN_TILT, route=route)


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


def deviation(got, want, where=""):
    """the measures of the module's docstring, worst over the batch; asserts what has to agree exactly"""
    assert np.array_equal(got["view_status"], want["view_status"]), (where, got["view_status"], want["view_status"])
    assert np.array_equal(got["cam_status"], want["cam_status"]), (where, got["cam_status"], want["cam_status"])
    assert np.array_equal(got["cam_views"], want["cam_views"]), (where, got["cam_views"], want["cam_views"])
    worst = dict(H=0.0, rows=0.0, fit_px=0.0, view_f=0.0, cam_f=0.0)
    for v in np.nonzero(want["view_status"] == ref.OK)[0]:
        assert got["view_used"][v] == want["view_used"][v], (where, v)
        Hg, Hw = np.asarray(got["view_H"][v]).reshape(3, 3), want["view_H"][v]
        Hg = Hg * np.sqrt(2.0 / (Hg[0, 0] ** 2 + Hg[1, 0] ** 2 + Hg[0, 1] ** 2 + Hg[1, 1] ** 2)) * np.sign((Hg * Hw).sum())
        worst["H"] = max(worst["H"], float(np.abs(Hg - Hw).max() / np.abs(Hw).max()))
        rg, rw = got["view_rows"][v], want["view_rows"][v]
        worst["rows"] = max(worst["rows"], _rel(rg[[0, 2]], rw[[0, 2]]), _rel(rg[[1, 3]], rw[[1, 3]]))
        worst["fit_px"] = max(worst["fit_px"], abs(got["view_fit_px"][v] - want["view_fit_px"][v]) / max(want["view_fit_px"][v], 0.01))
        assert np.isnan(got["view_f"][v]) == np.isnan(want["view_f"][v]), (where, v, got["view_f"][v], want["view_f"][v])
        if not np.isnan(want["view_f"][v]):
            worst["view_f"] = max(worst["view_f"], abs(got["view_f"][v] / want["view_f"][v] - 1.0))
    for c in np.nonzero(want["cam_status"] == ref.CAM_OK)[0]:
        worst["cam_f"] = max(worst["cam_f"], abs(got["cam_f"][c] / want["cam_f"][c] - 1.0))
    return worst


@functools.lru_cache(maxsize=None)
def bound():
    """(the bound, the spread of every group); asserts what the groups promise about the reference's output"""
    spreads = {}
    for name in GROUPS:
        g, r = group(name), reference(name)
        if "expect" in g:
            assert r["view_status"].tolist() == g["expect"], (name, r["view_status"])
        else:
            assert (r["view_status"] == ref.OK).all(), (name, r["view_status"])
        if "expect_cam" in g:
            assert r["cam_status"].tolist() == g["expect_cam"], (name, r["cam_status"])
        if "expect_used" in g:
            assert r["view_used"].tolist() == g["expect_used"], (name, r["view_used"])
        if "truth" in g:
            err = np.abs(r["cam_f"] / np.array(g["truth"]) - 1.0).max()
            assert err < 1e-8, (name, "the reference against the true focal length", err)
        if "cap" in g:
            assert abs(r["cam_f"][0] / g["cap"] - 1.0) < 0.25, (name, r["cam_f"][0], g["cap"])
        spreads[name] = max(deviation(reference(name, "svd"), r, name).values())
    b = 100.0 * max(spreads.values())
    assert b <= 1e-6, ("a case is too badly conditioned: replace it", spreads)
    fit = reference("fit_off")["view_fit_px"]
    assert fit[0] < 0.5 and fit[1] > 2.0, fit
    counts = reference("counts")
    assert counts["view_used"].tolist() == [0] + COUNTS[1:] + [63, 0]
    assert np.isnan(reference("cams")["view_f"][[1, 4, 7]]).all()          # the fronto-parallel views give no focal length of their own
    return b, spreads


def check(name, got, label=""):
    """got: the dict of vicalib_amd.lib.seed_focal_batch, run on arrays prefilled with FILL.  Prints the worst value / bound."""
    b, _ = bound()
    want = reference(name)
    worst = deviation(got, want, name)
    print("%s%s: bound %.3e; worst of value / bound -- H %.3e, rows %.3e, fit_px %.3e, view_f %.3e, cam_f %.3e"
          % (name, label, b, worst["H"] / b, worst["rows"] / b, worst["fit_px"] / b, worst["view_f"] / b, worst["cam_f"] / b))
    assert max(worst.values()) <= b, (name, worst, b)
    for v in np.nonzero(want["view_status"] != ref.OK)[0]:          # a refused view: the caller's values are still there
        assert np.all(got["view_H"][v] == FILL) and np.all(got["view_rows"][v] == FILL) and got["view_f"][v] == FILL and got["view_fit_px"][v] == FILL, (name, v)
        assert got["view_used"][v] == int(FILL), (name, v)
    for c in np.nonzero(want["cam_status"] != ref.CAM_OK)[0]:
        assert got["cam_f"][c] == FILL, (name, c)
    return worst


# ---------------------------------------------------------------------------------------------- the host build (tests/host_harness/seed_focal_harness.cpp)
def harness():
    src = os.path.join(HERE, "host_harness", "seed_focal_harness.cpp")
    so = os.path.join(HERE, "host_harness", "libvc_seed_focal_harness.so")
    deps = [src] + [os.path.join(ROOT, "vicalib_amd", "csrc", f) for f in ("vc_seed_focal.hpp", "vc_seed.hpp", "vc_undistort.hpp", "vc_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_run(g, keep=None, with_H=True):
    """the host build on the batch, in the layout of vicalib_amd.lib.seed_focal_batch, on prefilled outputs"""
    cam, pp, rad, off, pw, uv = batch_arrays(g, keep)
    n, nc = len(cam), len(rad)
    out = prefilled(n, nc)
    out.update(view_status=np.full(max(n, 1), -1, dtype=np.int32), cam_views=np.zeros(nc, dtype=np.int32), cam_status=np.full(nc, -1, dtype=np.int32))
    pw, uv = (pw if len(pw) else np.zeros((1, 3))), (uv if len(uv) else np.zeros((1, 2)))
    harness().seed_focal_harness_batch(n, _p(cam if n else np.zeros(1, dtype=np.int32)), nc, _p(np.ascontiguousarray(pp)), _p(rad), _p(off), _p(pw), _p(uv),
                                       int(g["min_corners"]), C.c_double(g["max_fit_px"]), C.c_double(g.get("min_tilt", MIN_TILT)), _p(out["view_H"]) if with_H else None,
                                       _p(out["view_rows"]), _p(out["view_f"]), _p(out["view_fit_px"]), _p(out["view_used"]), _p(out["view_status"]),
                                       _p(out["cam_f"]), _p(out["cam_views"]), _p(out["cam_status"]))
    out["view_status"] = out["view_status"][:n]
    return out


if __name__ == "__main__":
    b, spreads = bound()
    print("bound %.3e; spreads %s" % (b, {k: "%.2e" % v for k, v in spreads.items()}))
    for name in GROUPS:
        check(name, host_run(group(name)), label=" (host build)")
