"""TEST INFRASTRUCTURE: the rigs the rig seed (vc_seed_rig) is held to, shared by tests/test_seed_rig_cpu.py (the host build of vc_seed_rig.hpp,
tests/host_harness/seed_rig_harness.cpp) and tests/test_seed_rig_gpu.py (the kernels).  The reference is tests/seed_rig_ref.py, run once per
case and kept.

A case is poses built directly: a true rig (camera 0 into camera c), a true target-into-camera-0 pose per frame, every view the product of
the two with 0.2 degrees / 1 mm of noise, fixed seeds; a view that is not ok is NaN.  conditions() asserts on the reference what the groups
claim (winners, supports, parents) and that no comparison of any vote lies within 1e-9 relative of either threshold.

Tolerances (the issue's): statuses, shared, support, winner and parents exactly; pair_T_ab within 1e-12 on the quaternion and 1e-12 (1 + max |t|)
on the translation (sums of at most 257 terms of size <= 1: n eps = 6e-14); cam_T_c0 within 1e-11 (up to seven products); the two rms values at
rtol 1e-9, atol 1e-12."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import seed_rig_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PAIR_SIZES = (1, 2, 3, 63, 64, 65, 129, 257)
GROUPS = {
    "pair": ["pair_%d" % n for n in PAIR_SIZES],
    "flips": ["flips"], "tie": ["tie"], "signs": ["signs"], "chain": ["chain"], "tree_choice": ["tree_choice"], "island": ["island"], "few": ["few"], "eight": ["eight"],
}
MARGIN = 1e-9
F64_KEYS = ("pair_T_ab", "pair_rms_deg", "pair_rms_m", "cam_T_c0")
I32_KEYS = ("pair_shared", "pair_support", "pair_winner", "pair_status", "cam_parent", "cam_status")
FILL_F, FILL_I = 777.25, -5                      # what the prefilled buffers hold


# ------------------------------------------------------------------------------------------------ poses
def _rot(rng, max_deg, n=None):
    """rotation vectors with a uniform axis and an angle uniform in [-max_deg, max_deg]"""
    shape = (3,) if n is None else (n, 3)
    ax = rng.normal(size=shape); ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
    return ax * np.deg2rad(rng.uniform(-max_deg, max_deg, size=shape[:-1] + (1,)))


def _exp(w):
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def _M(R, t):
    M = np.eye(4); M[:3, :3] = R; M[:3, 3] = t
    return M


def rig(seed, n_cams):
    """camera 0 into camera c: up to 15 degrees, up to 0.2 m"""
    rng = np.random.default_rng(seed)
    return [np.eye(4)] + [_M(_exp(_rot(rng, 15.0)), rng.uniform(-0.2, 0.2, size=3)) for _ in range(n_cams - 1)]


def frames(seed, n):
    """the target into camera 0: up to 35 degrees off frontal, 0.5 .. 1 m away"""
    rng = np.random.default_rng(seed)
    return [_M(_exp(w), np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(0.5, 1.0)])) for w in _rot(rng, 35.0, n)]


def views(seed, T_c0, T_0w, ok, noise_deg=0.2, noise_m=1e-3):
    """view_ok [n, C] uint8, view_T [n, C, 7]: T_c0 T_0w(k) with noise on every view, NaN where ok is 0"""
    rng = np.random.default_rng(seed)
    n, nc = len(T_0w), len(T_c0)
    T = np.full((n, nc, 7), np.nan)
    for k in range(n):
        for c in range(nc):
            w = rng.normal(size=3); w *= np.deg2rad(noise_deg) * rng.normal() / np.linalg.norm(w)
            M = _M(_exp(w), rng.normal(scale=noise_m, size=3)) @ T_c0[c] @ T_0w[k]
            if ok[k, c]:
                T[k, c] = ref.matrix_to_pose(M)
    return np.ascontiguousarray(ok, dtype=np.uint8), T


def flip(T, rng, lo=20.0, hi=160.0):
    """the view turned by lo .. hi degrees about a random axis through the camera"""
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    return ref.matrix_to_pose(_M(_exp(ax * np.deg2rad(rng.uniform(lo, hi))), np.zeros(3)) @ ref.pose_to_matrix(T))


def _case(ok, T, T_c0=None, tol_deg=3.0, min_support=3, **extra):
    return dict(view_ok=ok, view_T=T, tol_deg=tol_deg, min_support=min_support, truth=T_c0, **extra)


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("pair_"):
        n = int(name[5:])
        ok, T = views(100 + n, rig(7, 2), frames(200 + n, n), np.ones((n, 2), dtype=bool))
        return _case(ok, T, rig(7, 2), min_support=1)
    if name == "flips":                                   # 30 % of the frames: camera 1's view 20 .. 160 degrees off
        n = 65
        ok, T = views(11, rig(8, 2), frames(12, n), np.ones((n, 2), dtype=bool))
        rng = np.random.default_rng(13)
        flipped = np.sort(rng.choice(n, size=int(round(0.3 * n)), replace=False))
        for k in flipped:
            T[k, 1] = flip(T[k, 1], rng)
        return _case(ok, T, rig(8, 2), flipped=flipped)
    if name == "tie":                                     # frames 0 and 1 alone, then two exact-duplicate clusters of 5, interleaved: frame 2 wins
        ok, T = views(21, rig(9, 2), frames(22, 4), np.ones((4, 2), dtype=bool), noise_deg=0.0, noise_m=0.0)
        rng = np.random.default_rng(23)
        one = [flip(T[0, 1], rng, 40.0, 60.0), flip(T[1, 1], rng, 80.0, 100.0)]
        two = flip(T[3, 1], rng, 120.0, 140.0)
        T12 = np.zeros((12, 2, 7))
        T12[0] = [T[0, 0], one[0]]; T12[1] = [T[1, 0], one[1]]
        for k in range(2, 12):
            T12[k] = [T[2, 0], T[2, 1]] if k % 2 == 0 else [T[3, 0], two]
        return _case(np.ones((12, 2), dtype=np.uint8), T12)
    if name == "signs":                                   # pair_65 with the quaternion of camera 1's view negated on odd frames
        c = case("pair_65")
        T = c["view_T"].copy()
        T[1::2, 1, :4] *= -1.0
        return _case(c["view_ok"], T, c["truth"], min_support=1)
    if name == "chain":                                   # 4 cameras sharing only 0-1, 1-2, 2-3
        ok = np.zeros((60, 4), dtype=bool)
        ok[0:20, 0:2] = True; ok[20:40, 1:3] = True; ok[40:60, 2:4] = True
        return _case(*views(31, rig(10, 4), frames(32, 60), ok), rig(10, 4))
    if name == "tree_choice":                             # supports 0-1: 40, 1-2: 50, 0-2: 10
        ok = np.zeros((100, 3), dtype=bool)
        ok[0:40, [0, 1]] = True; ok[40:90, [1, 2]] = True
        ok[90:100, 0] = True; ok[90:100, 2] = True
        return _case(*views(41, rig(11, 3), frames(42, 100), ok), rig(11, 3))
    if name == "island":                                  # camera 2 is seen only where nobody else is
        ok = np.zeros((30, 3), dtype=bool)
        ok[0:20, 0:2] = True; ok[20:30, 2] = True
        return _case(*views(51, rig(12, 3), frames(52, 30), ok), rig(12, 3))
    if name == "few":                                     # six shared frames, two of them agree: below min_support = 3
        ok, T = views(61, rig(13, 2), frames(62, 6), np.ones((6, 2), dtype=bool))
        rng = np.random.default_rng(63)
        for k, (lo, hi) in zip((0, 2, 3, 5), ((20, 30), (50, 60), (80, 90), (110, 120))):
            T[k, 1] = flip(T[k, 1], rng, lo, hi)
        return _case(ok, T, rig(13, 2))
    if name == "eight":                                   # 28 pairs, ragged visibility, a few flipped views
        n = 130
        rng = np.random.default_rng(71)
        ok = rng.uniform(size=(n, 8)) < 0.6
        ok[:, 0] |= rng.uniform(size=n) < 0.5
        ok, T = views(72, rig(14, 8), frames(73, n), ok)
        flipped = []
        for k in range(0, n, 9):
            c = 1 + (k // 9) % 7
            if ok[k, c]:
                T[k, c] = flip(T[k, c], rng); flipped.append((k, c))
        return _case(ok, T, rig(14, 8), flipped=flipped)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    return ref.seed(c["view_ok"], c["view_T"], c["tol_deg"], c["min_support"])


def conditions():
    """what the groups claim, asserted on the reference; returns the smallest margin"""
    margins = {}
    for names in GROUPS.values():
        for name in names:
            c, r = case(name), reference(name)
            margins[name] = r["margin"]
            assert r["margin"] >= MARGIN, (name, r["margin"])
            assert np.isnan(c["view_T"][c["view_ok"] == 0]).all()
    for n in PAIR_SIZES:
        r = reference("pair_%d" % n)
        assert r["pair_status"][0] == 0 and r["pair_shared"][0] == n == r["pair_support"][0] and list(r["cam_parent"]) == [-1, 0], n
    c, r = case("flips"), reference("flips")
    clean = 65 - len(c["flipped"])
    assert len(c["flipped"]) == 20 and r["pair_winner"][0] not in c["flipped"] and r["pair_support"][0] == clean and r["pair_status"][0] == 0
    assert set(r["pairs"][0]["members"]) == set(range(65)) - set(c["flipped"])
    r = reference("tie")
    assert list(r["pairs"][0]["all_support"]) == [1, 1] + [5] * 10 and r["pair_winner"][0] == 2 and r["pair_support"][0] == 5
    a, b = reference("pair_65"), reference("signs")
    assert np.abs(a["pair_T_ab"] - b["pair_T_ab"]).max() <= 1e-12 and a["pair_support"][0] == b["pair_support"][0] and a["pair_winner"][0] == b["pair_winner"][0]
    r = reference("chain")
    assert list(r["cam_parent"]) == [-1, 0, 1, 2] and list(r["pair_status"]) == [0, 1, 1, 0, 1, 0] and list(r["cam_status"]) == [0] * 4
    r = reference("tree_choice")
    assert list(r["pair_support"]) == [40, 10, 50] and list(r["cam_parent"]) == [-1, 0, 1]
    r = reference("island")
    assert list(r["pair_status"]) == [0, 1, 1] and list(r["cam_status"]) == [0, 0, 1] and list(r["cam_parent"]) == [-1, 0, -1]
    r = reference("few")
    assert list(r["pair_status"]) == [2] and r["pair_shared"][0] == 6 and r["pairs"][0]["all_support"].max() == 2 and list(r["cam_status"]) == [0, 1]
    c, r = case("eight"), reference("eight")
    assert (r["pair_status"] == 0).all() and (r["cam_status"] == 0).all() and len(c["flipped"]) >= 5 and (c["view_ok"] == 0).sum() > 200
    assert len(set(r["pair_shared"])) > 10 and r["pair_shared"].max() > 64                 # ragged, and more than one wavefront's stride
    # the reference finds the truth: every seeded pose within the noise of ONE candidate (two views at 0.2 degrees and 1 mm, 1 m from the target)
    for name in ("pair_257", "flips", "chain", "tree_choice", "eight"):
        c, r = case(name), reference(name)
        for cam, M in enumerate(c["truth"]):
            d = ref.pose_to_matrix(r["cam_T_c0"][cam]) @ np.linalg.inv(M)
            ang = np.rad2deg(np.arccos(min(1.0, 0.5 * (np.trace(d[:3, :3]) - 1.0))))
            assert ang < 0.3 and np.linalg.norm(r["cam_T_c0"][cam][4:] - M[:3, 3]) < 5e-3, (name, cam, ang)
    return margins


# ------------------------------------------------------------------------------------------------ the two builds
def harness():
    src = os.path.join(HERE, "host_harness", "seed_rig_harness.cpp")
    so = os.path.join(HERE, "host_harness", "libvc_seed_rig_harness.so")
    deps = [src] + [os.path.join(ROOT, "vicalib_amd", "csrc", f) for f in ("vc_seed_rig.hpp", "vc_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def prefilled(n_cams):
    P = n_cams * (n_cams - 1) // 2
    shapes = dict(pair_T_ab=(P, 7), pair_rms_deg=(P,), pair_rms_m=(P,), cam_T_c0=(n_cams, 7), pair_shared=(P,), pair_support=(P,), pair_winner=(P,), pair_status=(P,),
                  cam_parent=(n_cams,), cam_status=(n_cams,))
    return {k: (np.full(s, FILL_F) if k in F64_KEYS else np.full(s, FILL_I, dtype=np.int32)) for k, s in shapes.items()}


def constants():
    out = (C.c_int * 4)()
    harness().seed_rig_harness_constants(out)
    return dict(max_cams=out[0], max_frames=out[1], tile=out[2], record=out[3])


def host_seed_rig(view_ok, view_T, tol_deg, min_support):
    """the host build; the outputs start from prefilled()"""
    ok = np.ascontiguousarray(view_ok, dtype=np.uint8); T = np.ascontiguousarray(view_T, dtype=np.float64)
    o = prefilled(ok.shape[1])
    pad = {k: (v if v.size else np.zeros(1, dtype=v.dtype)) for k, v in o.items()}
    rc = harness().seed_rig_harness_run(ok.shape[0], ok.shape[1], _p(ok if ok.size else np.zeros(1, dtype=np.uint8)), _p(T if T.size else np.zeros(7)), C.c_double(tol_deg),
                                        int(min_support), _p(pad["pair_T_ab"]), _p(pad["pair_shared"]), _p(pad["pair_support"]), _p(pad["pair_winner"]),
                                        _p(pad["pair_rms_deg"]), _p(pad["pair_rms_m"]), _p(pad["pair_status"]), _p(pad["cam_T_c0"]), _p(pad["cam_parent"]), _p(pad["cam_status"]))
    assert rc == 0, rc
    return o


def device_seed_rig(view_ok, view_T, tol_deg, min_support):
    """the kernels, through the Python face; the outputs start from prefilled()"""
    import vicalib_amd.lib as lib
    return lib.seed_rig(view_ok, view_T, tol_deg=tol_deg, min_support=min_support, out=prefilled(np.asarray(view_ok).shape[1]))


# ------------------------------------------------------------------------------------------------ the checks
def compare(got, want, label):
    """`got` (outputs that started from prefilled()) against the reference `want`"""
    for k in ("pair_status", "pair_shared", "cam_parent", "cam_status"):
        assert np.array_equal(got[k], want[k]), (label, k, got[k], want[k])
    okp = want["pair_status"] == 0
    for k in ("pair_support", "pair_winner"):
        assert np.array_equal(got[k][okp], want[k][okp]), (label, k, got[k], want[k])
        assert (got[k][~okp] == FILL_I).all(), (label, k, "a refused pair's output was written")
    for k in ("pair_T_ab", "pair_rms_deg", "pair_rms_m"):
        assert (got[k][~okp] == FILL_F).all(), (label, k, "a refused pair's output was written")
    okc = want["cam_status"] == 0
    assert (got["cam_T_c0"][~okc] == FILL_F).all(), (label, "the pose of a camera that was not reached was written")
    worst = dict(q=0.0, t=0.0, cam=0.0, rms=0.0)
    if okp.any():
        g, w = got["pair_T_ab"][okp], want["pair_T_ab"][okp]
        worst["q"] = float(np.abs(g[:, :4] - w[:, :4]).max())
        worst["t"] = float((np.abs(g[:, 4:] - w[:, 4:]).max(axis=1) / (1.0 + np.abs(w[:, 4:]).max(axis=1))).max())
        for k in ("pair_rms_deg", "pair_rms_m"):
            worst["rms"] = max(worst["rms"], float((np.abs(got[k][okp] - want[k][okp]) / (1e-12 + 1e-9 * np.abs(want[k][okp]))).max()))
    worst["cam"] = float(np.abs(got["cam_T_c0"][okc] - want["cam_T_c0"][okc]).max())
    print("%s: quaternion %.2e translation %.2e (of 1e-12), cam_T_c0 %.2e (of 1e-11), rms %.2e of its tolerance" % (label, worst["q"], worst["t"], worst["cam"], worst["rms"]))
    assert worst["q"] <= 1e-12 and worst["t"] <= 1e-12 and worst["cam"] <= 1e-11 and worst["rms"] <= 1.0, (label, worst)
    return worst


def check(name, backend, label=""):
    c = case(name)
    got = backend(c["view_ok"], c["view_T"], c["tol_deg"], c["min_support"])
    compare(got, reference(name), name + label)
    return got


def check_signs(backend, label=""):
    a, b = check("pair_65", backend, label), check("signs", backend, label)
    assert np.abs(a["pair_T_ab"] - b["pair_T_ab"]).max() <= 1e-12 and np.abs(a["cam_T_c0"] - b["cam_T_c0"]).max() <= 1e-12, label
    assert a["pair_support"][0] == b["pair_support"][0] and a["pair_winner"][0] == b["pair_winner"][0]


def _bytes(r):
    return {k: r[k].tobytes() for k in F64_KEYS + I32_KEYS}


def check_bytes(backend):
    """two runs give the same bits; pair (0, 1) of `eight` gives the same bits with cameras 0 and 1 alone"""
    c = case("eight")
    a = backend(c["view_ok"], c["view_T"], c["tol_deg"], c["min_support"])
    b = backend(c["view_ok"], c["view_T"], c["tol_deg"], c["min_support"])
    assert _bytes(a) == _bytes(b)
    two = backend(np.ascontiguousarray(c["view_ok"][:, :2]), np.ascontiguousarray(c["view_T"][:, :2]), c["tol_deg"], c["min_support"])
    assert two["pair_status"][0] == 0 == a["pair_status"][0]
    for k in ("pair_T_ab", "pair_rms_deg", "pair_rms_m", "pair_shared", "pair_support", "pair_winner"):
        assert two[k][0].tobytes() == a[k][0].tobytes(), k
