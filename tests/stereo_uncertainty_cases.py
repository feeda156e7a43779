"""TEST INFRASTRUCTURE shared by test_stereo_uncertainty_cpu.py and test_stereo_uncertainty_gpu.py: the rigs, cameras and covariances of the
stereo uncertainty map, the numpy side of every check (the oracle's projection with its Jacobians, uncertainty_cases.jacobians, over the
rectified frames of rectify_cases.numpy_rotations) and the checks themselves -- written against plain arrays, so that the same check holds the
host build of the map's arithmetic (tests/host_harness/stereo_uncertainty_harness.cpp) and the GPU kernels.

A run is handed to the checks as a dict: var [n_depths, n, 3] = (var_dv, var_d, var_Z) and flags [n_depths, n] in sample order; summary, a list
per depth plane of dict(count, invalid, sum_var_dv, sum_var_d, sum_var_z, max_var_dv, worst); pose_var [7]; W [7, 12]."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import compare_cases as cc       # noqa: E402
import rectify_cases as rc       # noqa: E402
import uncertainty_cases as un   # noqa: E402
import undistort_cases as uc     # noqa: E402
from vicalib_amd import synth    # noqa: E402

SIZE = rc.SIZE                                    # of both cameras and of the rectified image
DST_LINEAR = rc.DST_LINEAR
GRID = (53, 41)                                   # 2173 samples: a partial wave, a partial workgroup
ONE_WORKGROUP = (64, 16)                          # exactly 1024 samples: four whole workgroups
TINY = (2, 2)
DEPTHS = (0.5, 2.0, 50.0)
MODEL_PAIRS = (("fov", "fov"), ("kb4", "poly3"), ("rational6", "poly2"), ("linear", "linear"))
NK = un.NK
FLAG_A, FLAG_B, FLAG_INVALID = cc.FLAG_A, cc.FLAG_B, cc.FLAG_INVALID
BORDER = 1e-9                                     # px: a pixel this close to an image border is undecided (one rounding of the projection decides)

# Check 1's tolerance.  MEASURED: the largest relative deviation of the host harness from the numpy reference over every case below -- of a
# variance against itself, of an entry of W against the largest of its row, of a pose variance against itself.  Printed by
# test_stereo_uncertainty_cpu.py (test_host_arithmetic, -s).  The bound is fifty times that (the convention of uncertainty_cases.MEASURED) and
# holds the device too.
MEASURED = 8.2e-14                                # linear / linear; every other case 2e-15 (2 x 2) to 7e-14
TOLERANCE = 50.0 * MEASURED


def exp_quat(T, w):
    """the pose T with q <- q * exp(w): the perturbation of vc_get_solution_covariance"""
    R, t = rc.pose_Rt(T)
    return rc.pose(R @ synth.so3_exp_matrix(np.asarray(w, dtype=np.float64)), t)


def quat_J(q):
    """the 4 x 3 matrix written out in vc_get_solution_covariance: dq = 1/2 J w for q <- q * exp(w), q = [x y z w]"""
    return np.array([[q[3], -q[2], q[1]], [q[2], q[3], -q[0]], [-q[1], q[0], q[3]], [-q[0], -q[1], -q[2]]])


@functools.lru_cache(maxsize=None)
def dense_cov(pair):
    """One dense covariance per pair in the layout of a two-camera rig's vc_get_solution_covariance, q_a (4) p_a (3) K_a q_b (4) p_b (3) K_b:
    Cov = (D L)(D L)^T with L lower triangular from numpy.random.default_rng(20261020 + index of the pair) -- row r: r draws of uniform(-1, 1),
    then the diagonal entry from uniform(0.5, 1), two decimals -- and D the plausible size of each parameter: 0.5e-3 for a quaternion entry
    (1e-3 rad), 1e-3 m for a translation, then uncertainty_cases.dense_cov's: 0.3 px for fu and fv, 0.5 px for u0 and v0, 1e-3 for a distortion
    term."""
    rng = np.random.default_rng(20261020 + MODEL_PAIRS.index(pair))
    nka, nkb = NK[pair[0]], NK[pair[1]]
    n = 14 + nka + nkb
    L = np.zeros((n, n))
    for r in range(n):
        L[r, :r] = np.round(rng.uniform(-1.0, 1.0, r), 2)
        L[r, r] = np.round(rng.uniform(0.5, 1.0), 2)
    side = lambda nk: [0.5e-3] * 4 + [1e-3] * 3 + [0.3, 0.3, 0.5, 0.5] + [1e-3] * (nk - 4)      # noqa: E731
    D = np.array(side(nka) + side(nkb))
    DL = D[:, None] * L
    return DL @ DL.T


class Case:
    def __init__(self, name, pair, grid=GRID, left=False, depths=DEPTHS):
        self.name, self.models, self.grid, self.depths = name, pair, grid, tuple(depths)
        self.K = [uc.gt(pair[0]), uc.gt(pair[1])]
        self.T_ck = list(rc.hand_rig(left))
        self.cov = dense_cov(pair)
        self.sigma_px = 1.0

    @property
    def cameras(self):
        return (self.models[0], self.K[0]), (self.models[1], self.K[1])


def case_names():
    return ["%s-%s" % p for p in MODEL_PAIRS] + ["left", "one-workgroup", "tiny"]


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "left":
        return Case(name, ("fov", "fov"), left=True)
    if name == "one-workgroup":
        return Case(name, ("kb4", "poly3"), grid=ONE_WORKGROUP)
    if name == "tiny":
        return Case(name, ("kb4", "poly3"), grid=TINY)
    return Case(name, tuple(name.split("-")))


# ------------------------------------------------------------------------------------------------------------ numpy reference
def numpy_pose_jacobian(T_ck_a, T_ck_b):
    """W [7, 12] = d(w_a, w_b, baseline) / d(w_ck_a, dp_a, w_ck_b, dp_b) of rectify_cases.numpy_rotations, the issue's closed form in numpy"""
    Rak, _ = rc.pose_Rt(T_ck_a)
    _, tb = rc.pose_Rt(T_ck_b)
    R, _, c = rc.relative(T_ck_a, T_ck_b)
    Rda, _, b = rc.numpy_rotations(T_ck_a, T_ck_b)
    e1, e2, e3 = Rda
    g = R.T @ tb
    zb = R.T @ np.eye(3)[2]
    zm = np.eye(3)[2] + zb
    n2 = np.linalg.norm(np.cross(zm, e1))
    W = np.zeros((7, 12))
    for col in range(12):
        d = np.zeros(12); d[col] = 1.0
        phi = Rak @ (d[6:9] - d[0:3])
        dc = -np.cross(g, phi) + d[3:6] - R.T @ d[9:12]
        de1 = np.sign(b) * (dc - e1 * (e1 @ dc)) / abs(b)
        du = np.cross(np.cross(zb, phi), e1) + np.cross(zm, de1)
        de2 = (du - e2 * (e2 @ du)) / n2
        de3 = np.cross(de1, e2) + np.cross(e1, de2)
        wa = np.array([de3 @ e2, de1 @ e3, de2 @ e1])
        W[0:3, col], W[3:6, col], W[6, col] = wa, wa - Rda @ phi, e1 @ dc
    return W


def numeric_pose_jacobian(T_ck_a, T_ck_b, h=1e-4):
    """the same by central differences of numpy_rotations with one Richardson step (error of order h^4)"""
    Ra0, Rb0, _ = rc.numpy_rotations(T_ck_a, T_ck_b)

    def out(d):
        Ta = exp_quat(T_ck_a, d[0:3]); Ta[4:] += d[3:6]
        Tb = exp_quat(T_ck_b, d[6:9]); Tb[4:] += d[9:12]
        Ra, Rb, b = rc.numpy_rotations(Ta, Tb)
        return np.concatenate([un.rotation_vector(Ra @ Ra0.T), un.rotation_vector(Rb @ Rb0.T), [b]])

    def central(step):
        return np.stack([(out(step * e) - out(-step * e)) / (2.0 * step) for e in np.eye(12)], 1)
    return (4.0 * central(0.5 * h) - central(h)) / 3.0


def eta_map(T_ck_a, T_ck_b, nka, nkb, W):
    """T [27, n]: eta = [w_a, w_b, db, dK_a (10), dK_b (10)] per unit of the ambient parameters"""
    n = 14 + nka + nkb
    T = np.zeros((27, n))
    for c, (Tck, first) in enumerate(((T_ck_a, 0), (T_ck_b, 7 + nka))):
        T[:7, first:first + 4] = W[:, 6 * c:6 * c + 3] @ (2.0 * quat_J(Tck[:4]).T)
        T[:7, first + 4:first + 7] = W[:, 6 * c + 3:6 * c + 6]
    T[7:7 + nka, 7:7 + nka] = np.eye(nka)
    T[17:17 + nkb, 14 + nka:] = np.eye(nkb)
    return T


def _side(model, K, R_ds, dl, r, size):
    """one side at the rectified points r [n, 3]: pix [n, 2], ok [n], near [n] (the pixel within BORDER of an image border), the block
    [n, 2, 13] (zero where not ok)"""
    n, nk = len(r), NK[model]
    a = r @ R_ds
    front = (a[:, 2] > 0) | (model == "kb4")
    pix, A, B = np.full((n, 2), np.nan), np.zeros((n, 2, 3)), np.zeros((n, 2, nk))
    if front.any():
        with np.errstate(all="ignore"):
            pix[front], A[front], B[front] = un.jacobians(model, K, a[front])
    lim = np.array([size[0] - 1.0, size[1] - 1.0])
    with np.errstate(invalid="ignore"):
        ok = front & np.isfinite(pix).all(1) & (pix >= 0).all(1) & (pix <= lim).all(1)
        near = front & ((np.abs(pix) <= BORDER).any(1) | (np.abs(pix - lim) <= BORDER).any(1))
    blk = np.zeros((n, 2, 13))
    k = np.nonzero(ok)[0]
    Ak, Bk, rk = A[k], B[k], r[k]
    da = -np.einsum("nji,njk,nkl->nil", Ak, np.linalg.inv(np.einsum("nij,nkj->nik", Ak, Ak)), Bk)      # -A^T (A A^T)^-1 B: [n, 3, nk]
    Pi = np.zeros((len(k), 2, 3))
    Pi[:, 0, 0], Pi[:, 0, 2] = dl[0] / rk[:, 2], -dl[0] * rk[:, 0] / rk[:, 2] ** 2
    Pi[:, 1, 1], Pi[:, 1, 2] = dl[1] / rk[:, 2], -dl[1] * rk[:, 1] / rk[:, 2] ** 2
    blk[k, :, :3] = -np.einsum("nij,njk->nik", Pi, un.cross_matrix(rk))
    blk[k, :, 3:3 + nk] = np.einsum("nij,jk,nkl->nil", Pi, R_ds, da)
    return pix, ok, near, blk


class Reference:
    """of one pair on one lattice at some depths: q, R_ds, baseline, W, T; per depth pix (2), ok (2), valid, undecided and the rows J [n, 3, 27]"""

    def __init__(self, models, K, T_ck, grid, depths, dl=DST_LINEAR, size=SIZE, dst_size=SIZE):
        self.models, self.K, self.T_ck, self.grid, self.depths, self.dl = models, [np.asarray(k, dtype=np.float64) for k in K], T_ck, grid, tuple(depths), np.asarray(dl)
        self.q, _ = cc.lattice(dst_size, grid)
        self.Ra, self.Rb, self.b = rc.numpy_rotations(T_ck[0], T_ck[1])
        self.W = numpy_pose_jacobian(T_ck[0], T_ck[1])
        self.T = eta_map(T_ck[0], T_ck[1], NK[models[0]], NK[models[1]], self.W)
        self.pix, self.ok, self.valid, self.undecided, self.J = [], [], [], [], []
        n = len(self.q)
        for Z in self.depths:
            P = np.stack([(self.q[:, 0] - dl[2]) * Z / dl[0], (self.q[:, 1] - dl[3]) * Z / dl[1], np.full(n, Z)], 1)
            pa, oka, na, ba = _side(models[0], self.K[0], self.Ra, dl, P, size)
            pb, okb, nb, bb = _side(models[1], self.K[1], self.Rb, dl, P - [self.b, 0.0, 0.0], size)
            d = dl[0] * self.b / Z
            J = np.zeros((n, 3, 27))
            for row, o in ((0, 1), (1, 0)):                          # dv from the v rows, d from the u rows
                J[:, row, 0:3], J[:, row, 3:6] = ba[:, o, :3], -bb[:, o, :3]
                J[:, row, 7:17], J[:, row, 17:27] = ba[:, o, 3:], -bb[:, o, 3:]
            J[:, 2] = -(Z / d) * J[:, 1]
            J[:, 2, 6] = dl[0] / d
            self.pix.append((pa, pb)); self.ok.append((oka, okb)); self.valid.append(oka & okb); self.undecided.append(na | nb); self.J.append(J)

    def cov_eta(self, cov, sigma_px=1.0):
        return sigma_px ** 2 * self.T @ np.asarray(cov) @ self.T.T

    def triples(self, cov, sigma_px=1.0):
        """[n_depths, n, 3], NaN where not valid"""
        C = self.cov_eta(cov, sigma_px)
        out = []
        for J, valid in zip(self.J, self.valid):
            t = np.einsum("nrk,kl,nrl->nr", J, C, J)
            t[~valid] = np.nan
            out.append(t)
        return np.stack(out)


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    return Reference(c.models, c.K, c.T_ck, c.grid, c.depths)


def check_shares(ref):
    """the condition on a 53 x 41 case, under the numpy reference alone: per depth at least a third of the samples valid and at least 5 %
    invalid; at most 1 % undecided"""
    for Z, valid, und in zip(ref.depths, ref.valid, ref.undecided):
        print("depth %g: valid share %.3f, undecided %d" % (Z, valid.mean(), und.sum()))
        assert valid.mean() >= 1.0 / 3.0 and (~valid).mean() >= 0.05, (Z, valid.mean())
        assert und.mean() <= 0.01


# ------------------------------------------------------------------------------------------------------------ checks
def deviation(ref, cov, sigma_px, out):
    """Check 1 without its bound: the flags exactly on decided samples, then the largest relative deviation of every variance valid on both
    sides (against itself), of W (per entry, against the largest of its row) and of the pose variances"""
    var, flags = np.asarray(out["var"]).reshape(len(ref.depths), -1, 3), np.asarray(out["flags"]).reshape(len(ref.depths), -1)
    t = ref.triples(cov, sigma_px)
    dev = 0.0
    for k in range(len(ref.depths)):
        dec = ~ref.undecided[k]
        oka, okb = ref.ok[k]
        assert np.array_equal(((flags[k] & FLAG_A) != 0)[dec], ~oka[dec]) and np.array_equal(((flags[k] & FLAG_B) != 0)[dec], ~okb[dec])
        bad = (flags[k] & FLAG_INVALID) != 0
        assert np.array_equal(bad[dec], ~ref.valid[k][dec]) and np.all(bad[(flags[k] & (FLAG_A | FLAG_B)) != 0])
        assert not (flags[k].astype(int) & ~(FLAG_A | FLAG_B | FLAG_INVALID)).any()
        assert np.isnan(var[k][bad]).all() and np.isfinite(var[k][~bad]).all()
        both = dec & ~bad & ref.valid[k]
        if np.any(t[k][both] > 0):
            assert (t[k][both] > 0).all()
            dev = max(dev, (np.abs(var[k][both] - t[k][both]) / t[k][both]).max())
        else:
            assert not np.any(var[k][both])
    dev = max(dev, (np.abs(out["W"] - ref.W) / np.abs(ref.W).max(axis=1, keepdims=True)).max())
    pv = np.diag(ref.cov_eta(cov, sigma_px))[:7]
    if np.any(pv > 0):
        dev = max(dev, (np.abs(out["pose_var"] - pv) / pv).max())
    else:
        assert not np.any(out["pose_var"])
    return float(dev)


def check_map(ref, cov, sigma_px, out, name=""):
    """1. every valid sample's triple, W and the pose variances against numpy; flags equal on decided samples"""
    dev = deviation(ref, cov, sigma_px, out)
    print("%s: largest relative deviation from numpy %.3g (bound %.3g)" % (name, dev, TOLERANCE))
    assert dev <= TOLERANCE
    return dev


def check_sums(ref, cov, sigma_px, out):
    """2. the summary of every depth plane against numpy sums over the reference's own triples (at an undecided sample the run's own flag and
    triple), with check 1's tolerance; the worst sample is the first of the largest var_dv -- the dense covariances must leave the top two
    apart by more than the tolerance (a CPU precondition)"""
    var, flags = np.asarray(out["var"]).reshape(len(ref.depths), -1, 3), np.asarray(out["flags"]).reshape(len(ref.depths), -1)
    t = ref.triples(cov, sigma_px)
    for k, s in enumerate(out["summary"]):
        und = ref.undecided[k]
        ok = np.where(und, (flags[k] & FLAG_INVALID) == 0, ref.valid[k])
        tk = t[k].copy()
        tk[und & ok] = var[k][und & ok]
        assert s["count"] == ok.sum() and s["invalid"] == (~ok).sum()
        if not ok.any():
            assert s["worst"] == -1 and s["max_var_dv"] == 0 and s["sum_var_dv"] == 0 and s["sum_var_d"] == 0 and s["sum_var_z"] == 0
            continue
        for key, col in (("sum_var_dv", 0), ("sum_var_d", 1), ("sum_var_z", 2)):
            assert abs(s[key] - tk[ok, col].sum()) <= TOLERANCE * tk[ok, col].sum(), (k, key)
        top = np.sort(tk[ok, 0])[-2:]
        assert abs(s["max_var_dv"] - top[-1]) <= TOLERANCE * top[-1]
        if len(top) == 2 and np.any(np.asarray(cov)):
            assert top[1] - top[0] > TOLERANCE * top[1], (top, TOLERANCE)
        assert s["worst"] == np.nonzero(ok)[0][np.argmax(tk[ok, 0])]
        # ... and exactly the first of the run's own largest values
        assert s["worst"] == np.nanargmax(np.where((flags[k] & FLAG_INVALID) == 0, var[k][:, 0], -1.0)) and s["max_var_dv"] == var[k][s["worst"], 0]


def check_case(name, run):
    """Checks 1 and 2 of one case.  run(case, cov, sigma_px, depths) -> the dict above."""
    c, ref = case(name), reference(name)
    out = run(c, c.cov, c.sigma_px, c.depths)
    dev = check_map(ref, c.cov, c.sigma_px, out, name)
    check_sums(ref, c.cov, c.sigma_px, out)
    return out, dev


def same_bits(a, b, scale=1.0):
    """every output of run a times `scale` equals that of run b bit for bit (NaN where NaN); the flags, counts and worst samples equal"""
    eq = lambda x, y: np.array_equal(np.asarray(x) * scale, np.asarray(y), equal_nan=True)      # noqa: E731
    ok = eq(a["var"], b["var"]) and np.array_equal(a["flags"], b["flags"]) and eq(a["pose_var"], b["pose_var"]) and len(a["summary"]) == len(b["summary"])
    for sa, sb in zip(a["summary"], b["summary"]):
        ok = ok and all(sa[k] == sb[k] for k in ("count", "invalid", "worst")) and all(eq(sa[k], sb[k]) for k in ("sum_var_dv", "sum_var_d", "sum_var_z", "max_var_dv"))
    return bool(ok)


def plane(out, k):
    """depth plane k of a run as a run of its own"""
    return dict(var=np.asarray(out["var"])[k:k + 1], flags=np.asarray(out["flags"])[k:k + 1], summary=out["summary"][k:k + 1], pose_var=out["pose_var"], W=out["W"])


def swapped(c, Z):
    """case c at depth Z with A and B exchanged, on the same points: (cameras, T_ck, dst_linear, cov).  B's rectified frame is A's moved by the
    baseline, so a principal point moved by the disparity fu b / Z puts the swapped lattice on the same points; dv changes its sign."""
    ref = reference(c.name)
    dl = DST_LINEAR.copy(); dl[2] += dl[0] * ref.b / Z
    na = 7 + NK[c.models[0]]
    perm = np.concatenate([np.arange(na, len(c.cov)), np.arange(na)])
    return (c.cameras[1], c.cameras[0]), (c.T_ck[1], c.T_ck[0]), dl, c.cov[np.ix_(perm, perm)]


# ------------------------------------------------------------------------------------------------------------ the semantic pin
# (what is perturbed, its index, delta, the numpy gaps max | |dv| - sqrt(var_dv) | and max | |d - d0| - sqrt(var_d) | in px over the valid samples
# of the kb4 / poly3 pair on the 53 x 41 lattice at the three depths).  "Ka" / "Kb": intrinsic k of that side; "wb" / "pb": component k of the
# rotation (q <- q * exp(delta e_k)) and of the translation of B's pose.
PIN_PAIR = ("kb4", "poly3")
# Halving delta divides every gap by 3.99 to 4.02: they are the second order of the shift.
PIN = (("Ka", 4, 1e-3, 2.11e-3, 3.01e-3), ("Kb", 2, 0.1, 1.02e-5, 2.83e-5), ("wb", 1, 1e-3, 2.30e-4, 4.49e-4), ("pb", 0, 1e-3, 1.12e-3, 3.82e-4))


def pin_perturbed(what, k, delta):
    """(K [2], T_ck [2], the ambient covariance delta^2 e e^T) of the perturbed calibration of the pin's pair"""
    c = case("%s-%s" % PIN_PAIR)
    K, T = [c.K[0].copy(), c.K[1].copy()], [c.T_ck[0].copy(), c.T_ck[1].copy()]
    nka = NK[c.models[0]]
    e = np.zeros(len(c.cov))
    if what == "Ka":
        K[0][k] += delta; e[7 + k] = delta
    elif what == "Kb":
        K[1][k] += delta; e[14 + nka + k] = delta
    elif what == "wb":
        T[1] = exp_quat(T[1], delta * np.eye(3)[k]); e[7 + nka:11 + nka] = 0.5 * delta * quat_J(c.T_ck[1][:4])[:, k]
    else:
        T[1][4 + k] += delta; e[11 + nka + k] = delta
    return K, T, np.outer(e, e)


class _Pairs:
    pass


@functools.lru_cache(maxsize=None)
def pin_numpy(what, k, delta):
    """numpy's side of the pin: the pixels p_a, p_b of every valid sample re-rectified at the perturbed calibration (rectify_cases.reference_pairs)
    -> per depth (|dv| [n], |d - d0| [n], use [n]: valid and re-rectified), and the two gaps against the reference's own first order"""
    c, ref = case("%s-%s" % PIN_PAIR), reference("%s-%s" % PIN_PAIR)
    K, T, cov = pin_perturbed(what, k, delta)
    t = ref.triples(cov)
    planes, gaps = [], np.zeros(2)
    for i, Z in enumerate(ref.depths):
        p = _Pairs()
        p.models, p.K, p.T_ck = c.models, K, T
        v = ref.valid[i] & ~ref.undecided[i]
        p.px_a, p.px_b = ref.pix[i][0][v], ref.pix[i][1][v]
        pairs, bad = rc.reference_pairs(p, dl=DST_LINEAR)
        dv, dd, use = np.full(len(v), np.nan), np.full(len(v), np.nan), v.copy()
        dv[v], dd[v] = np.abs(pairs[:, 0]), np.abs(pairs[:, 1] - DST_LINEAR[0] * ref.b / Z)
        use[v] = ~bad
        planes.append((dv, dd, use))
        gaps = np.maximum(gaps, [np.abs(dv[use] - np.sqrt(t[i][use, 0])).max(), np.abs(dd[use] - np.sqrt(t[i][use, 1])).max()])
    return planes, gaps


def check_pin(what, k, delta, tabulated, out, planes, gaps=None):
    """3. rank-one covariance at sigma_px 1: sqrt(var_dv) against |dv| and sqrt(var_d) against |d - d0| of the re-rectified pixels (numpy's on the
    CPU, a real Rectifier's on the GPU) within 1.5 x the numpy gap + 1e-7 px.  gaps: numpy's own, held to the table within a tenth (the CPU
    test); None: the table's (the GPU test, which does not repeat numpy's bisections)"""
    if gaps is not None:
        assert np.all(np.abs(gaps - tabulated) <= 0.1 * np.asarray(tabulated)), (what, k, gaps, tabulated)
    gaps = np.asarray(tabulated, dtype=np.float64)
    var = np.asarray(out["var"]).reshape(len(planes), -1, 3)
    for i, (dv, dd, use) in enumerate(planes):
        got = [float(np.abs(np.sqrt(var[i][use, col]) - x[use]).max()) for col, x in ((0, dv), (1, dd))]
        print("%s %d, plane %d: |sqrt(var_dv) - |dv|| %.3g px (bound %.3g), |sqrt(var_d) - |d - d0|| %.3g px (bound %.3g), largest |dv| %.3g, |d - d0| %.3g px"
              % (what, k, i, got[0], 1.5 * gaps[0] + 1e-7, got[1], 1.5 * gaps[1] + 1e-7, dv[use].max(), dd[use].max()))
        assert got[0] <= 1.5 * gaps[0] + 1e-7 and got[1] <= 1.5 * gaps[1] + 1e-7
