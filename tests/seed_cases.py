"""The views the batched planar PnP (vc_pnp_planar_batch, vc_seed.hpp) is held to, shared by tests/test_seed_cpu.py (the host build of its
arithmetic, tests/host_harness/seed_harness.cpp) and tests/test_seed_gpu.py (the kernel).  The reference is the host routine the device path
replaces: pnp_planar / pnp_planar_ransac of vicalib_amd.lib, run once per group and kept.

A group is a batch: one iteration count and one tolerance for all its views.
  plain        iterations 0: 4, 5, 8, 63, 64, 65, 190 corners (the minimum; the smallest that would enter the robust branch; one corner per
               lane and one either side; a full board, three rounds per lane), a view on the plane z = 0.37, a noiseless full view of each
               of the six models, and the refusals a 3-corner view (status 1) and a view with one corner off the plane (status 2)
  robust       iterations 100, tol 1 px: 5 (noiseless, no mismatch), 8, 63, 64, 65, 190, 12, 190 (z = -0.2), 64 corners over all six
               models; sigma 0.05 px; max(1, n // 5) corners of every view of >= 8 carry another dot's detection, moved by >= 3 px
  its1 / its64 / its65   the robust views at the iteration counts either side of one hypothesis per lane, and a single hypothesis
  noise        iterations 100, tol 0.5 px: a view whose pixels are unrelated noise (status 4) beside a good one

Band condition (a condition on the INPUT, not a measurement): at the host's returned pose no correspondence of a robust view has an error in
(tol / 2, 2 tol).  Which of two near-tied hypotheses wins, and the rounding of a sum, then cannot move the final set: the re-vote of the
refined pose converges to it.  host_reference() asserts the condition on the host's output; a view that violates it gets another seed, the
band stays.

Tolerances: the project's parameter tolerances (top of tests/test_holdout_gpu.py) -- rotation 1e-6 rad, translation 1e-6 relative with a floor
of 1e-9 m, rms 1e-6 relative with a floor of 1e-9 px; the inlier mask exactly.  The host stops at a relative cost decrease of 1e-12, which at
0.05 px noise and f = 300 px leaves it about 1e-10 rad from the optimum: two right implementations are four orders inside the bound."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from vicalib_amd import synth
from vicalib_amd.lib import VicalibError, pnp_planar_ransac

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODELS = ["fov", "poly2", "poly3", "kb4", "linear", "rational6"]
COUNTS = [4, 5, 8, 63, 64, 65, 190]
ROBUST_COUNTS = [5, 8, 63, 64, 65, 190, 12, 190, 64]
SIGMA, TOL = 0.05, 1.0
OK, FEW, NOT_PLANAR, NO_POSE, NO_CONSENSUS = range(5)
GROUPS = ["plain", "robust", "its1", "its64", "its65", "noise"]


def _inv(T):
    R = synth.quat_to_matrix(T[:4])
    return synth.se3_from_Rt(R.T, -R.T @ T[4:])


def _mul(A, B):
    Ra, Rb = synth.quat_to_matrix(A[:4]), synth.quat_to_matrix(B[:4])
    return synth.se3_from_Rt(Ra @ Rb, Ra @ B[4:] + A[4:])


def pose_distance(Ta, Tb):
    """(|t_a - t_b|, angle of R_a^T R_b in radians); the vector part of the relative rotation: exact to first order for tiny angles"""
    Ra, Rb = synth.quat_to_matrix(np.asarray(Ta)[:4]), synth.quat_to_matrix(np.asarray(Tb)[:4])
    dR = Ra.T @ Rb
    w = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) * 0.5
    return float(np.linalg.norm(np.asarray(Ta)[4:] - np.asarray(Tb)[4:])), float(np.arcsin(min(1.0, np.linalg.norm(w))))


@functools.lru_cache(maxsize=None)
def _problem(model, sigma, seed):
    return synth.generate(synth.Config(models=(model,), n_frames=10, seed=seed, pixel_sigma=sigma))


def _view(name, model, n, seed, sigma=SIGMA, z0=0.0, mismatch=False, tile=None):
    """n corners of one tile of a synthetic problem; T_gt is the generating T_cw (for the plane the view is moved to)"""
    p = _problem(model, sigma, seed)
    if n is None:                                                             # the fullest view there is
        n = max(len(t[2]) for t in p.tiles)
    tiles = [t for t in p.tiles if len(t[2]) >= n]
    assert tiles, (name, model, n, seed)
    f, c, ids, pix = tiles[(seed if tile is None else tile) % len(tiles)]
    rng = np.random.default_rng(1000 * seed + n)
    keep = np.sort(rng.choice(len(ids), size=n, replace=False))
    pw, uv = p.grid_points[ids[keep]].copy(), pix[keep].copy()
    changed = np.zeros(n, dtype=bool)
    if mismatch:
        bad = rng.choice(n, size=max(1, n // 5), replace=False)
        src = (bad + 2 + rng.integers(0, n - 4, size=len(bad))) % n           # another dot's detection
        moved = uv.copy()
        moved[bad] = uv[src]
        changed = np.linalg.norm(moved - uv, axis=1) >= 3.0
        assert changed[bad].all(), (name, "a mismatched corner moved by less than 3 px")
        uv = moved
    T_cw = _mul(p.cam_T_ck_gt[c], _inv(p.frame_T_wk_gt[f]))
    if z0 != 0.0:                                                             # the same pixels seen from a target on the plane z = z0
        pw[:, 2] += z0
        T_cw = T_cw.copy()
        T_cw[4:] -= synth.quat_to_matrix(T_cw[:4])[:, 2] * z0
    return dict(name=name, model=model, K=np.asarray(p.cam_K_gt[c], dtype=np.float64), pw=np.ascontiguousarray(pw), uv=np.ascontiguousarray(uv),
                expect=OK, T_gt=T_cw, noiseless=sigma == 0.0 and not mismatch, changed=changed)


# per robust view: (model, seed); a view that breaks the band condition gets another seed here
_ROBUST_SEEDS = [("linear", 3), ("fov", 5), ("poly2", 7), ("poly3", 11), ("kb4", 13), ("rational6", 17), ("linear", 19), ("kb4", 23), ("fov", 29)]


def _robust_views():
    out = []
    for k, (n, (model, seed)) in enumerate(zip(ROBUST_COUNTS, _ROBUST_SEEDS)):
        if n == 5:      # noiseless and unmixed: with noise every four-point sample fits itself exactly and the tie-break falls to rounding
            out.append(_view("robust-5-%s" % model, model, 5, seed, sigma=0.0))
        else:
            out.append(_view("robust-%d-%s%s" % (n, model, "-z" if k == 7 else ""), model, n, seed, z0=-0.2 if k == 7 else 0.0, mismatch=True))
    return out


@functools.lru_cache(maxsize=None)
def group(name):
    """dict(its, tol, views)"""
    if name == "plain":
        views = [_view("plain-%d-%s" % (n, MODELS[k % 6]), MODELS[k % 6], n, 31 + k) for k, n in enumerate(COUNTS)]
        views.append(_view("plain-190-kb4-z", "kb4", 190, 41, z0=0.37))
        views += [_view("noiseless-%s" % m, m, None, 3, sigma=0.0) for m in MODELS]
        few = _view("three-corners", "poly3", 4, 43)
        few.update(pw=few["pw"][:3].copy(), uv=few["uv"][:3].copy(), expect=FEW, changed=few["changed"][:3])
        bent = _view("not-planar", "fov", 64, 47)
        bent["pw"][17, 2] += 0.05
        bent["expect"] = NOT_PLANAR
        return dict(its=0, tol=0.0, views=views + [few, bent])
    if name in ("robust", "its1", "its64", "its65"):
        return dict(its={"robust": 100, "its1": 1, "its64": 64, "its65": 65}[name], tol=TOL, views=_robust_views())
    if name == "noise":
        junk = _view("unrelated-noise", "poly3", 64, 53)
        rng = np.random.default_rng(9)
        junk["uv"] = np.ascontiguousarray(np.stack([rng.uniform(5, 635, 64), rng.uniform(5, 475, 64)], axis=1))
        junk["expect"] = NO_CONSENSUS
        return dict(its=100, tol=0.5, views=[junk, _view("noise-good-kb4", "kb4", 65, 59, sigma=0.0)])
    raise KeyError(name)


def errors(view, T):
    """reprojection error of every correspondence at T_cw, by the generator's projection"""
    R = synth.quat_to_matrix(np.asarray(T)[:4])
    pc = view["pw"] @ R.T + np.asarray(T)[4:]
    pix = synth.project(synth.MODEL_IDS[view["model"]], view["K"], pc)
    return np.linalg.norm(pix - view["uv"], axis=1)


@functools.lru_cache(maxsize=None)
def host_reference(name):
    """the host routine on every view of the group, once: list of dict(ok, T, rms, inlier); asserts what the group promises about its input"""
    g = group(name)
    out = []
    for v in g["views"]:
        try:
            T, rms, inl = pnp_planar_ransac(v["model"], v["K"], v["pw"], v["uv"], iterations=g["its"], tol_px=g["tol"])
            out.append(dict(ok=True, T=T, rms=rms, inlier=inl))
        except VicalibError:
            out.append(dict(ok=False, T=None, rms=None, inlier=np.zeros(len(v["pw"]), dtype=bool)))
        r = out[-1]
        if v["expect"] == OK and name in ("robust", "its1", "its64", "its65") and not r["ok"]:
            continue                             # (a single hypothesis may find no consensus: the refusal is then the thing compared)
        assert r["ok"] == (v["expect"] == OK), (name, v["name"], "the host routine disagrees with the case's expectation")
        if r["ok"] and g["its"] > 0 and len(v["pw"]) >= 5:
            e = errors(v, r["T"])
            band = (e > 0.5 * g["tol"]) & (e < 2.0 * g["tol"])
            assert not band.any(), (name, v["name"], "band condition: errors %s in (tol / 2, 2 tol); change this view's seed" % e[band])
    return out


def check_against_host(name, got, label=""):
    """got: status [n], T_cw [n, 7], rms [n], n_inliers [n], inlier (list of bool arrays, one per view).  Prints the worst value / bound."""
    g, ref = group(name), host_reference(name)
    worst = dict(rot=0.0, t=0.0, rms=0.0, truth=0.0)
    for k, (v, r) in enumerate(zip(g["views"], ref)):
        st = int(got["status"][k])
        if not r["ok"]:          # the host returned false: the listed status, or (a robust view at a single hypothesis) one of the two it can mean
            assert st == v["expect"] if v["expect"] != OK else st in (NO_POSE, NO_CONSENSUS), (name, v["name"], st)
            assert not np.asarray(got["inlier"][k]).any(), (name, v["name"], "flags of a refused view")
            continue
        assert st == OK, (name, v["name"], st)
        assert np.array_equal(np.asarray(got["inlier"][k], dtype=bool), r["inlier"]), (name, v["name"], "inlier mask")
        assert int(got["n_inliers"][k]) == int(r["inlier"].sum()), (name, v["name"])
        dt, dr = pose_distance(got["T_cw"][k], r["T"])
        worst["rot"] = max(worst["rot"], dr / 1e-6)
        worst["t"] = max(worst["t"], dt / max(1e-6 * np.linalg.norm(r["T"][4:]), 1e-9))
        worst["rms"] = max(worst["rms"], abs(got["rms"][k] - r["rms"]) / max(1e-6 * r["rms"], 1e-9))
        if v["noiseless"]:
            T = np.asarray(got["T_cw"][k])
            sgn = np.sign(T[:4] @ v["T_gt"][:4])
            worst["truth"] = max(worst["truth"], float(np.abs(T[:4] * sgn - v["T_gt"][:4]).max()) / 1e-7, float(np.abs(T[4:] - v["T_gt"][4:]).max()) / 1e-7)
    print("%s%s: worst of value / bound -- rotation %.3e, translation %.3e, rms %.3e, generating pose of the noiseless views %.3e"
          % (name, label, worst["rot"], worst["t"], worst["rms"], worst["truth"]))
    assert worst["rot"] <= 1.0 and worst["t"] <= 1.0 and worst["rms"] <= 1.0 and worst["truth"] <= 1.0


def batch_arrays(views):
    """(models, params, view_off, p_w, p_c) of vicalib_amd.lib.pnp_planar_batch"""
    off = np.concatenate([[0], np.cumsum([len(v["pw"]) for v in views])]).astype(np.int32)
    return ([v["model"] for v in views], [v["K"] for v in views], off, np.concatenate([v["pw"] for v in views]), np.concatenate([v["uv"] for v in views]))


def split(off, flags):
    return [flags[off[k]:off[k + 1]] for k in range(len(off) - 1)]


# ---------------------------------------------------------------------------------------------- the host build (tests/host_harness/seed_harness.cpp)
def harness():
    src = os.path.join(HERE, "host_harness", "seed_harness.cpp")
    so = os.path.join(HERE, "host_harness", "libvc_seed_harness.so")
    deps = [src] + [os.path.join(ROOT, "vicalib_amd", "csrc", f) for f in ("vc_seed.hpp", "vc_undistort.hpp", "vc_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_seed(name):
    """the host build of the device arithmetic on every view of the group, serially, in the layout check_against_host takes"""
    g, H = group(name), harness()
    n = len(g["views"])
    got = dict(status=np.zeros(n, dtype=np.int32), T_cw=np.full((n, 7), -7.0), rms=np.full(n, -7.0), n_inliers=np.full(n, -7, dtype=np.int32), inlier=[])
    for k, v in enumerate(g["views"]):
        K = np.zeros(10); K[:len(v["K"])] = v["K"]
        flags = np.zeros(len(v["pw"]), dtype=np.int8)
        n_in = C.c_int(-7); rms = C.c_double(-7.0)
        got["status"][k] = H.seed_harness_view(synth.MODEL_IDS[v["model"]], _p(K), len(v["pw"]), _p(v["pw"]), _p(v["uv"]), g["its"], C.c_double(g["tol"]),
                                               _p(got["T_cw"][k]), C.byref(rms), C.byref(n_in), _p(flags))
        got["rms"][k], got["n_inliers"][k] = rms.value, n_in.value
        got["inlier"].append(flags.astype(bool))
    return got


def host_picks(n, its):
    table = np.zeros((its, 4), dtype=np.int32)
    harness().seed_harness_picks(int(n), int(its), _p(table))
    return table


def contract_picks(n, its):
    """the pick sequence as the contract states it (splitmix64 from 0x9E3779B97F4A7C15 ^ n, next() % n, a repeated pick redrawn), in Python integers"""
    mask = (1 << 64) - 1
    state = 0x9E3779B97F4A7C15 ^ n
    table = np.zeros((its, 4), dtype=np.int32)
    for it in range(its):
        pick = []
        while len(pick) < 4:
            state = (state + 0x9E3779B97F4A7C15) & mask
            z = state
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
            z ^= z >> 31
            if z % n not in pick:
                pick.append(z % n)
        table[it] = pick
    return table


if __name__ == "__main__":
    for name in GROUPS:
        check_against_host(name, host_seed(name), label=" (host build)")
