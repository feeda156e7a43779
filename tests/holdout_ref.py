"""Host restatement (float64) of the per-frame problem of the held-out scoring: a helper of the hold-out tests, not a test.

One held-out frame, cameras frozen: minimise  1/2 sum_i rho(|r_i|^2)  over the 6 parameters of the rig pose T_wk, rho = SoftLOne(0.5)
(rho(s) = 2 b (sqrt(1 + s / b) - 1) with b = 0.25, the function of loss_soft_l1), r_i = project(R_ck R_wk^T (p_w - t_wk) + t_ck) - z_i
over every corner of every view of the frame.  Projection and its derivative come from the CPU oracle (oracle_lib.project), which is
independent of the device arithmetic; the pose Jacobian is derived here from T <- T exp([v, w]):
    p_k' = exp(-w)(p_k - V v) ~ p_k - v + p_k x w      =>      d p_c / d [v, w] = R_ck [-I | [p_k]x]
The solver is an own damped Gauss-Newton / Levenberg-Marquardt with the exact gradient sum rho' J^T r; it is driven until the gradient
max-norm is at most `gtol_rel` times the one at the start.  A corner at camera-frame depth <= 0 enters no sum, as on the device.
"""
import ctypes as C

import numpy as np

import oracle_lib as ol
from vicalib_amd.synth import quat_from_matrix, quat_to_matrix, so3_exp_matrix

SOFT_L1_B = 0.25


def rho(s):
    """SoftLOne(0.5): (rho, rho')."""
    t = np.sqrt(1.0 + s / SOFT_L1_B)
    return 2.0 * SOFT_L1_B * (t - 1.0), 1.0 / t


def _hat(p):
    return np.array([[0.0, -p[2], p[1]], [p[2], 0.0, -p[0]], [-p[1], p[0], 0.0]])


def se3_exp_apply(T, d):
    """T * exp([v, w]) for T = [qx qy qz qw tx ty tz]."""
    T = np.asarray(T, dtype=np.float64); d = np.asarray(d, dtype=np.float64)
    v, w = d[:3], d[3:]
    th = np.linalg.norm(w)
    W = _hat(w)
    if th > 1e-6:
        a = (1.0 - np.cos(th)) / th ** 2; b = (th - np.sin(th)) / th ** 3
    else:
        a = 0.5 - th ** 2 / 24.0; b = 1.0 / 6.0 - th ** 2 / 120.0
    V = np.eye(3) + a * W + b * (W @ W)
    R = quat_to_matrix(T[:4])
    Rn = R @ so3_exp_matrix(w)
    q = quat_from_matrix(Rn)
    if np.dot(q, T[:4]) < 0:
        q = -q
    return np.concatenate([q, T[4:] + R @ (V @ v)])


class Frame:
    """The views of one held-out frame: cams = [(model id, K, T_ck)], views = [(camera, p_w [n, 3], pix [n, 2])]."""

    def __init__(self, cams, views):
        self.cams = [(int(m), np.ascontiguousarray(K, dtype=np.float64), np.asarray(T, dtype=np.float64)) for (m, K, T) in cams]
        self.views = [(int(c), np.asarray(pw, dtype=np.float64).reshape(-1, 3), np.asarray(px, dtype=np.float64).reshape(-1, 2)) for (c, pw, px) in views]

    def n_corners(self):
        return sum(len(pw) for (_, pw, _) in self.views)

    def residuals(self, T, jac=False):
        """r [n, 2] in view order (NaN rows for corners at depth <= 0) and, with jac, J [n, 2, 6].  The projection is the oracle's
        vco_project, the function oracle_lib.project wraps, called on preallocated buffers."""
        T = np.asarray(T, dtype=np.float64)
        Rwk = quat_to_matrix(T[:4]); twk = T[4:]
        L = ol.lib()
        pix = np.zeros(2); dray = np.zeros((2, 3)); dk = np.zeros((2, 16)); ray = np.zeros(3)
        a_pix, a_dray, a_dk, a_ray = (x.ctypes.data_as(C.c_void_p) for x in (pix, dray, dk, ray))
        rs, Js = [], []
        for (c, pw, px) in self.views:
            m, K, Tck = self.cams[c]
            a_K = K.ctypes.data_as(C.c_void_p)
            Rck = quat_to_matrix(Tck[:4]); tck = Tck[4:]
            pk = (pw - twk) @ Rwk                     # rows R_wk^T (p_w - t_wk)
            pc = pk @ Rck.T + tck
            r = np.full((len(pw), 2), np.nan); A = np.zeros((len(pw), 2, 3))
            for i in np.nonzero(pc[:, 2] > 0.0)[0]:
                ray[:] = pc[i]
                L.vco_project(m, a_ray, a_K, a_pix, a_dray, a_dk)
                r[i] = pix - px[i]; A[i] = dray
            rs.append(r)
            if jac:
                AR = A @ Rck                          # d pix / d p_k
                hat = np.zeros((len(pw), 3, 3))
                hat[:, 0, 1] = -pk[:, 2]; hat[:, 0, 2] = pk[:, 1]; hat[:, 1, 0] = pk[:, 2]; hat[:, 1, 2] = -pk[:, 0]; hat[:, 2, 0] = -pk[:, 1]; hat[:, 2, 1] = pk[:, 0]
                Js.append(np.concatenate([-AR, AR @ hat], axis=2))
        r = np.concatenate(rs) if rs else np.zeros((0, 2))
        return (r, np.concatenate(Js) if Js else np.zeros((0, 2, 6))) if jac else r

    def cost(self, T):
        r = self.residuals(T)
        r = r[~np.isnan(r[:, 0])]
        return 0.5 * rho((r * r).sum(axis=1))[0].sum()

    def linearize(self, T):
        """cost, gradient (6), Gauss-Newton matrix (6 x 6) with the first-order robust weights."""
        r, J = self.residuals(T, jac=True)
        ok = ~np.isnan(r[:, 0])
        r, J = r[ok], J[ok]
        p, w = rho((r * r).sum(axis=1))
        g = np.einsum("n,nij,ni->j", w, J, r)
        H = np.einsum("n,nij,nik->jk", w, J, J)
        return 0.5 * p.sum(), g, H

    def gradient_max_norm(self, T):
        return float(np.abs(self.linearize(T)[1]).max())


def refine(frame, T0, gtol_rel=1e-12, max_iters=300):
    """-> (T, info): damped Gauss-Newton from T0 until max |g| <= gtol_rel * max |g(T0)|; info = dict(converged, iterations, g0, g, cost).
    A step is taken when it lowers the cost; close to the optimum, where the decrease g^2 / H drowns in the rounding of the cost, when it
    leaves the cost where it is to rounding and lowers the gradient max-norm."""
    T = np.asarray(T0, dtype=np.float64).copy()
    cost, g, H = frame.linearize(T)
    g0 = float(np.abs(g).max())
    lam = 1e-4
    it = 0
    while it < max_iters and np.abs(g).max() > gtol_rel * g0:
        it += 1
        try:
            d = -np.linalg.solve(H + lam * np.diag(np.diag(H)), g)
        except np.linalg.LinAlgError:
            lam *= 10.0
            continue
        Tn = se3_exp_apply(T, d)
        cn, gn, Hn = frame.linearize(Tn)
        if np.isfinite(cn) and (cn < cost * (1.0 - 1e-13) or (cn <= cost * (1.0 + 1e-13) and np.abs(gn).max() < np.abs(g).max())):
            T, cost, g, H = Tn, cn, gn, Hn
            lam = max(lam * 0.1, 1e-15)
        else:
            lam *= 10.0
            if lam > 1e12:
                break
    gm = float(np.abs(g).max())
    return T, dict(converged=gm <= gtol_rel * g0, iterations=it, g0=g0, g=gm, cost=float(cost))


def pose_distance(Ta, Tb):
    """(|t_a - t_b|, angle of q_a^-1 q_b in radians)."""
    Ra, Rb = quat_to_matrix(np.asarray(Ta)[:4]), quat_to_matrix(np.asarray(Tb)[:4])
    dR = Ra.T @ Rb
    w = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) * 0.5      # sin(angle) * axis: exact to first order for tiny angles
    return float(np.linalg.norm(np.asarray(Ta)[4:] - np.asarray(Tb)[4:])), float(np.arcsin(min(1.0, np.linalg.norm(w))))


def frames_of(prob_cams, grid_points, tiles, frame_ids):
    """Frame objects of the held-out frames `frame_ids` out of a synthetic problem's tiles [(frame, cam, dot ids, pix)]."""
    out = []
    for f in frame_ids:
        out.append(Frame(prob_cams, [(c, grid_points[ids], px) for (ff, c, ids, px) in tiles if ff == f]))
    return out
