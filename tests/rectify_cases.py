"""TEST INFRASTRUCTURE shared by test_rectify_cpu.py and test_rectify_gpu.py: the rigs, the matched corner pairs cut from the synthetic
generator, the numpy side of every comparison (the oracle's projection inverted by bisection, Kabsch by SVD with explicit residuals;
computed once per case and kept) and the checks themselves -- written against plain arrays, so that the same check holds the host build of
the check's arithmetic (tests/host_harness/rectify_harness.cpp) and the GPU kernel."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import undistort_cases as uc     # noqa: E402
from vicalib_amd import synth    # noqa: E402

MODEL_PAIRS = (("fov", "fov"), ("kb4", "poly3"), ("rational6", "poly2"))
FRAME_SIZES = (0, 1, 2, 3, 5, 63, 64, 65, 130, 190)      # lane-stride tails, a last workgroup that is not full (10 frames, 4 per workgroup)
SIZE = (640, 480)
DST_LINEAR = np.array([300.0, 300.0, 319.5, 239.5])
IDENTITY_POSE = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def pose(R, t):
    return synth.se3_from_Rt(np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64))


def pose_Rt(T):
    return synth.quat_to_matrix(np.asarray(T[:4])), np.asarray(T[4:], dtype=np.float64)


def relative(T_ck_a, T_ck_b):
    """(R, t, c): p_b = R p_a + t and the centre of b in a's frame"""
    Ra, ta = pose_Rt(T_ck_a); Rb, tb = pose_Rt(T_ck_b)
    R = Rb @ Ra.T
    t = tb - R @ ta
    return R, t, -R.T @ t


# ------------------------------------------------------------------------------------------------------------ rigs
@functools.lru_cache(maxsize=None)
def generator_rig(models):
    p = synth.generate(synth.Config(models=models, n_frames=2, pixel_sigma=0.0))
    return p.cam_T_ck_gt[0].copy(), p.cam_T_ck_gt[1].copy()


def hand_rig(left=False):
    """camera b 12 cm to the right of a (left=True: to the left), a little forward and down, turned by 10 degrees about an oblique axis; a itself
    sits off the rig's origin"""
    Ra = uc.rotation((2.0, -3.0, 1.5)); ta = np.array([0.02, -0.01, 0.03])
    Rrel = synth.so3_exp_matrix(np.deg2rad(10.0) * np.array([0.3, 0.8, 0.52]) / np.linalg.norm([0.3, 0.8, 0.52]))
    c = np.array([-0.12 if left else 0.12, 0.015, 0.02])
    # p_b = Rrel (p_a - c)
    return pose(Ra, ta), pose(Rrel @ Ra, Rrel @ (ta - c))


def vertical_rig():
    return IDENTITY_POSE.copy(), pose(np.eye(3), [0.01, -0.1, 0.0])


def rigs():
    return {"fov-fov": generator_rig(("fov", "fov")), "kb4-poly3": generator_rig(("kb4", "poly3")), "hand": hand_rig(), "hand-left": hand_rig(True)}


def check_rotations(T_ck_a, T_ck_b, R_ds_a, R_ds_b, baseline, tol=1e-12):
    """orthonormal, determinant + 1; R_ds_b p_b - R_ds_a p_a = (-b, 0, 0) for random points; upright"""
    for M in (R_ds_a, R_ds_b):
        assert np.abs(M @ M.T - np.eye(3)).max() <= tol and abs(np.linalg.det(M) - 1.0) <= tol
    R, t, c = relative(T_ck_a, T_ck_b)
    pa = np.random.default_rng(5).uniform(-1.0, 1.0, (64, 3)) + [0, 0, 2.0]
    pb = pa @ R.T + t
    diff = pb @ R_ds_b.T - pa @ R_ds_a.T
    assert np.abs(diff - [-baseline, 0.0, 0.0]).max() <= tol, np.abs(diff - [-baseline, 0.0, 0.0]).max()
    xm = np.eye(3)[0] + R.T @ np.eye(3)[0]
    assert R_ds_a[0] @ xm > 0.0
    assert abs(abs(baseline) - np.linalg.norm(c)) <= tol


# ------------------------------------------------------------------------------------------------------------ matched pairs
@functools.lru_cache(maxsize=None)
def problem(models, sigma, intrinsics=None):
    return synth.generate(synth.Config(models=models, n_frames=12, pixel_sigma=sigma, gt_intrinsics=intrinsics))


def common_corners(prob, frame):
    """(ids, pix_a, pix_b) of the corners cameras 0 and 1 both see in `frame`, by numpy.intersect1d"""
    t = {c: (ids, pix) for (f, c, ids, pix) in prob.tiles if f == frame}
    ids, ia, ib = np.intersect1d(t[0][0], t[1][0], return_indices=True)
    return ids, t[0][1][ia], t[1][1][ib]


def camera_points(prob, frame, cam, ids):
    """ground truth: the target points `ids` in the frame of camera `cam`"""
    Rwk, twk = pose_Rt(prob.frame_T_wk_gt[frame]); Rck, tck = pose_Rt(prob.cam_T_ck_gt[cam])
    return ((prob.grid_points[ids] - twk) @ Rwk) @ Rck.T + tck


class Case:
    """models, K (2), T_ck (2), frame_off, px_a, px_b, target, p_a (ground truth in camera a's frame)"""


def cut(prob, sizes, keep=None, seed=3):
    """Frame k of the case holds sizes[k] common corners of one of the problem's frames (a random subset in point-id order).  The frames with
    the most common corners are used, the largest size on the richest frame: the rational6 / poly2 rig has a frame of 185 common corners,
    fewer than the largest size."""
    rng = np.random.default_rng(seed)
    usable = [common_corners(prob, f) for f in range(prob.cfg.n_frames)]
    if keep is not None:
        usable = [tuple(v[keep(camera_points(prob, f, 0, u[0]))] for v in u) for f, u in enumerate(usable)]
    richest = np.argsort([len(u[0]) for u in usable], kind="stable")[-len(sizes):]
    frame_of = richest[np.argsort(np.argsort(sizes, kind="stable"), kind="stable")]
    c = Case()
    c.models = prob.cfg.models
    c.K = [np.array(k, dtype=np.float64) for k in prob.cam_K_gt]
    c.T_ck = [prob.cam_T_ck_gt[0].copy(), prob.cam_T_ck_gt[1].copy()]
    off, A, B, X, PA = [0], [], [], [], []
    for k, n in zip(frame_of, sizes):
        ids, pa, pb = usable[k]
        assert len(ids) >= n, (k, len(ids), n)
        sel = np.sort(rng.choice(len(ids), n, replace=False))
        A.append(pa[sel]); B.append(pb[sel]); X.append(prob.grid_points[ids[sel]]); PA.append(camera_points(prob, k, 0, ids[sel]))
        off.append(off[-1] + n)
    c.frame_off = np.array(off, dtype=np.int64)
    c.px_a, c.px_b, c.target, c.p_a = (np.concatenate(v).reshape(-1, w) for v, w in ((A, 2), (B, 2), (X, 3), (PA, 3)))
    return c


@functools.lru_cache(maxsize=None)
def check_case(models, sigma):
    return cut(problem(models, sigma), FRAME_SIZES)


@functools.lru_cache(maxsize=None)
def beyond_case():
    """Side a is undistort_cases.BEYOND_K, whose image ends at a radius of 198.76 px; the corners are those within r_u < 0.5 of a's axis, well
    inside it.  Frames of 5, 65 and 64 pairs; in the 65-pair frame pair 7's pixel in a is moved to 1.5 times that radius."""
    models = ("poly3", "fov")
    prob = problem(models, 0.1, (tuple(uc.BEYOND_K), tuple(uc.gt("fov"))))
    c = cut(prob, (5, 65, 64), keep=lambda p: np.hypot(p[:, 0], p[:, 1]) / p[:, 2] < 0.5)
    c.bad = np.array([c.frame_off[1] + 7])
    c.px_a = c.px_a.copy()
    c.px_a[c.bad[0]] = uc.BEYOND_K[2:4] + 1.5 * 198.76 * np.array([0.6, -0.8])
    return c


@functools.lru_cache(maxsize=None)
def swapped_case():
    """the noisy kb4 / poly3 case with the two pixels of pair 11 of the 65-pair frame exchanged: a disparity of the wrong sign"""
    src = check_case(("kb4", "poly3"), 0.1)
    c = Case()
    c.__dict__.update(src.__dict__)
    c.bad = np.array([c.frame_off[7] + 11])
    c.px_a, c.px_b = src.px_a.copy(), src.px_b.copy()
    c.px_a[c.bad[0]], c.px_b[c.bad[0]] = src.px_b[c.bad[0]], src.px_a[c.bad[0]]
    return c


# ------------------------------------------------------------------------------------------------------------ numpy reference
def numpy_rotations(T_ck_a, T_ck_b):
    """the issue's construction, in numpy"""
    R, t, c = relative(T_ck_a, T_ck_b)
    I = np.eye(3)
    e1 = c / np.linalg.norm(c)
    xm, zm = I[0] + R.T @ I[0], I[2] + R.T @ I[2]
    if e1 @ xm < 0:
        e1 = -e1
    e2 = np.cross(zm, e1); e2 /= np.linalg.norm(e2)
    Ra = np.stack([e1, e2, np.cross(e1, e2)])
    return Ra, Ra @ R.T, float(e1 @ c)


@functools.lru_cache(maxsize=None)
def t_limit(model, K):
    """the end of the bracket the bisection starts from: where the oracle's profile stops increasing (BEYOND_K), at most the field's edge"""
    K = np.array(K)
    t = np.linspace(0.0, 1.5 if model == "kb4" else 2.0, 601)
    r = uc.profile(model, K, t)
    up = np.nonzero(np.diff(r) <= 0)[0]
    return float(t[up[0]] if len(up) else t[-1])


def unproject_many(model, K, px):
    """oracle-side inverse of every pixel [n, 2] by bisection on the oracle's profile (undistort_cases.profile), all pixels at once: rays [n, 3]
    and whether the pixel's radius is inside the profile's range"""
    d = (np.asarray(px, dtype=np.float64) - K[2:4]) / K[:2]
    rd = np.hypot(d[:, 0], d[:, 1])
    hi0 = t_limit(model, tuple(K))
    inside = rd < uc.profile(model, K, np.array([hi0]))[0]
    lo, hi = np.zeros(len(rd)), np.full(len(rd), hi0)
    for _ in range(56):
        mid = 0.5 * (lo + hi)
        below = uc.profile(model, K, mid) < rd
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return uc.ray_at(model, 0.5 * (lo + hi), np.arctan2(d[:, 1], d[:, 0])), inside


def kabsch_rms(P, X):
    """RMS residual of the best rotation + translation (no scale) of P onto X: SVD, residuals evaluated explicitly"""
    p, x = P - P.mean(0), X - X.mean(0)
    U, _, Vt = np.linalg.svd(p.T @ x)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return float(np.sqrt(np.sum((p @ R.T - x) ** 2) / len(P)))


def reference_pairs(c, T_ck=None, dl=DST_LINEAR):
    """(pairs [n, 6], invalid [n]) of a case by the issue's arithmetic in numpy"""
    T = c.T_ck if T_ck is None else T_ck
    Ra, Rb, b = numpy_rotations(T[0], T[1])
    out = []
    ok = np.ones(len(c.px_a), dtype=bool)
    for model, K, R, px in ((c.models[0], c.K[0], Ra, c.px_a), (c.models[1], c.K[1], Rb, c.px_b)):
        rays, inside = unproject_many(model, K, px)
        r = rays @ R.T
        ok &= inside & (r[:, 2] > 0)
        with np.errstate(all="ignore"):
            out.append(np.stack([dl[0] * r[:, 0] / r[:, 2] + dl[2], dl[1] * r[:, 1] / r[:, 2] + dl[3]], 1))
    (ua, va), (ub, vb) = out[0].T, out[1].T
    d = ua - ub
    ok &= d * b > 0
    with np.errstate(all="ignore"):
        Z = dl[0] * b / d
        vm = 0.5 * (va + vb)
        pairs = np.stack([va - vb, d, (ua - dl[2]) * Z / dl[0], (vm - dl[3]) * Z / dl[1], Z, vm], 1)
    pairs[~ok] = np.nan
    return pairs, ~ok


@functools.lru_cache(maxsize=None)
def reference(name, models=None):
    c = {"beyond": beyond_case, "swapped": swapped_case}[name]() if models is None else check_case(models, 0.1)
    return reference_pairs(c)


# ------------------------------------------------------------------------------------------------------------ checks
def frames_of(c):
    return [slice(int(c.frame_off[k]), int(c.frame_off[k + 1])) for k in range(len(c.frame_off) - 1)]


def check_frame_rows(c, out, with_target=True):
    """Every per-frame value against numpy over the SAME run's per-pair outputs.  Sums: 1e-12 relative -- for sum dv, whose terms cancel,
    relative to sum |dv| (a sum of n terms carries n eps sum |x| at the most; n <= 190, eps = 1.1e-16); the maximum and the counts exactly; the
    rigid fit against Kabsch on the run's own P at 1e-9 relative + 1e-12 m."""
    pairs, bad = out["pairs"], np.asarray(out["invalid"], dtype=bool)
    assert np.all(np.isnan(pairs[bad])) and np.all(np.isfinite(pairs[~bad]))
    for k, s in enumerate(frames_of(c)):
        good = ~bad[s]
        dv, P = pairs[s][good, 0], pairs[s][good, 2:5]
        assert out["count"][k] == good.sum() and out["n_invalid"][k] == (~good).sum(), k
        if good.sum() == 0:
            assert out["sum_dv"][k] == 0 and out["sum_dv2"][k] == 0 and out["max_abs_dv"][k] == 0 and out["mean_z"][k] == 0 and out["worst"][k] == -1
            assert np.isnan(out["rigid_rms"][k])
            continue
        assert abs(out["sum_dv"][k] - dv.sum()) <= 1e-12 * np.abs(dv).sum(), k
        assert abs(out["sum_dv2"][k] - (dv ** 2).sum()) <= 1e-12 * (dv ** 2).sum(), k
        assert abs(out["mean_z"][k] - P[:, 2].mean()) <= 1e-12 * abs(P[:, 2].mean()), k
        assert out["max_abs_dv"][k] == np.abs(dv).max(), k
        assert out["worst"][k] == s.start + np.nonzero(good)[0][np.argmax(np.abs(dv))], k      # argmax: the first of equal maxima
        if with_target and good.sum() >= 3:
            want = kabsch_rms(P, c.target[s][good])
            assert abs(out["rigid_rms"][k] - want) <= 1e-9 * want + 1e-12, (k, out["rigid_rms"][k], want)
        else:
            assert np.isnan(out["rigid_rms"][k]), k


def check_pairs_against_reference(out, ref_pairs, ref_bad):
    """flags equal; dv, d and the mean row at 1e-8 px, P at 1e-9 m; returns the two largest differences"""
    bad = np.asarray(out["invalid"], dtype=bool)
    assert np.array_equal(bad, ref_bad), np.nonzero(bad != ref_bad)[0][:5]
    diff = np.abs(out["pairs"][~bad] - ref_pairs[~bad])
    e_px, e_m = diff[:, [0, 1, 5]].max(), diff[:, 2:5].max()
    assert e_px <= 1e-8 and e_m <= 1e-9, (e_px, e_m)
    return e_px, e_m


def check_exact(c, out, R_ds_a):
    """pixel_sigma = 0 and the ground-truth cameras: rows line up, the triangulated corners are the corners, the rigid fit has nothing left"""
    assert not np.asarray(out["invalid"]).any()
    e_dv = np.abs(out["pairs"][:, 0]).max()
    e_p = np.abs(out["pairs"][:, 2:5] - c.p_a @ np.asarray(R_ds_a).T).max()
    rms = out["rigid_rms"][np.asarray(out["count"]) >= 3]
    assert e_dv <= 1e-9 and e_p <= 1e-9 and rms.max() <= 1e-9, (e_dv, e_p, rms.max())
    return e_dv, e_p, rms.max()
