"""A numpy restatement of the target step (include/vicalib_amd.h: vc_target_refine_batch, vicalib_amd/csrc/vc_target_refine.hpp), for the tests of
the host build and of the kernels.  One Gauss-Newton step on the target's points with the frame poses and the shared camera columns marginalised,
by two routes:

  (a) "normal"  the marginalised normal equations as the definition states them: per frame J^T J - W^T H_ff^-1 W over [s | d], s eliminated with
                the scaled, 1e-6-regularised S_ss, then (Pi M Pi + mu Q Q^T) d = Pi b;
  (b) "lstsq"   one numpy.linalg.lstsq on the stacked, UNSQUARED Jacobian over [frame poses | s | z] with d = Pi z, the rows
                sqrt(lambda) (Pi (points - nominal) + Pi z) and the rows sqrt(1e-6) / c_j s_j appended; predicted_decrease is the difference of
                the linear model's minimum without and with the target columns.

The spread between the two is the conditioning of a case.  The rows of a corner are the analytic ones of tests/select_ref.py plus J_p = A R_cw;
rows_numeric() restates them by central differences of vicalib_amd.synth's projection -- no closed form."""
import numpy as np

import select_ref as sref
from vicalib_amd import synth

PRIOR_S = 1e-6
GAUGE_TOL = 1e-9
PIVOT_TOL = 1e-12
OK, SINGULAR = 0, 1


def views_of(case):
    """{frame: [(camera, point ids, measurements)] ordered by camera, a camera's tiles concatenated in the order of arrival}"""
    per = {}
    for f, c, ids, z in case["tiles"]:
        e = per.setdefault(f, {}).setdefault(c, ([], []))
        e[0].extend(int(i) for i in ids); e[1].extend(np.asarray(z, dtype=np.float64).reshape(-1, 2).tolist())
    return {f: [(c, np.array(v[c][0], dtype=int), np.array(v[c][1], dtype=np.float64).reshape(-1, 2)) for c in sorted(v)] for f, v in per.items()}


def _geometry(case, f, c):
    m, K, T_ck, flags = case["cameras"][c]
    T = np.asarray(case["poses"][f], dtype=np.float64)
    Rwk, twk = sref.quat_R(T, np.float64), T[4:7]
    Rck, tck = sref.quat_R(T_ck, np.float64), np.asarray(T_ck[4:7], dtype=np.float64)
    return sref.model_id(m), np.asarray(K, dtype=np.float64), flags, Rwk, twk, Rck, tck


def rows_analytic(case, f, c, ids, z):
    """(J_f [2n, 6], J_c [2n, camera's columns], J_p [n, 2, 3], r [2n], in front [n]) of one view; the first two are tests/select_ref.py's"""
    m, K, flags, Rwk, twk, Rck, tck = _geometry(case, f, c)
    Jf, Jc, front = sref.analytic_rows(case, f, c, ids, np.float64)
    pw = np.asarray(case["points"], dtype=np.float64)[ids][front]
    pc = (pw - twk) @ Rwk @ Rck.T + tck
    A, _ = sref._proj_jac(m, K, pc, np.float64)
    Jp = A @ (Rck @ Rwk.T)
    with np.errstate(all="ignore"):
        r = (synth.project(m, K, pc) - z[front]).reshape(-1)
    return Jf, Jc, Jp, r, front


def rows_numeric(case, f, c, ids, z, h):
    """the same Jacobians by central differences of step h"""
    m, K, flags, Rwk, twk, Rck, tck = _geometry(case, f, c)
    Jf, Jc, front = sref.numeric_rows(case, f, c, ids, h)
    pw = np.asarray(case["points"], dtype=np.float64)[ids][front]

    def pix(dp):
        with np.errstate(all="ignore"):
            return synth.project(m, K, (pw + dp - twk) @ Rwk @ Rck.T + tck)
    Jp = np.stack([(pix(e * h) - pix(-e * h)) / (2 * h) for e in np.eye(3)], axis=2)
    return Jf, Jc, Jp, (pix(np.zeros(3)) - z[front]).reshape(-1), front


def frame_rows(case, rows=rows_analytic):
    """per frame: dict(Jf [2n, 6], Js [2n, D], Jp [2n, 3P], r [2n]), status, corners, behind, and the usable corners of every point"""
    cams = case["cameras"]
    N, P, D = len(case["poses"]), len(case["points"]), sref.dim(cams)
    col0 = np.cumsum([0] + [sref.ncols(c[0], c[3]) for c in cams])
    views = views_of(case)
    out, status, corners, behind = [], np.zeros(N, dtype=int), np.zeros(N, dtype=int), np.zeros(N, dtype=int)
    pcorners = np.zeros(P, dtype=int)
    for f in range(N):
        Jfs, Jss, Jps, rs, seen = [np.zeros((0, 6))], [np.zeros((0, D))], [np.zeros((0, 3 * P))], [np.zeros(0)], []
        for c, ids, z in views.get(f, []):
            Jf, Jc, Jp, r, front = rows(case, f, c, ids, z)
            corners[f] += int(front.sum()); behind[f] += int((~front).sum())
            Js = np.zeros((len(Jf), D)); Js[:, col0[c]:col0[c + 1]] = Jc
            Jd = np.zeros((len(Jf), 3 * P))
            for k, p in enumerate(ids[front]):
                Jd[2 * k:2 * k + 2, 3 * p:3 * p + 3] = Jp[k]
            Jfs.append(Jf); Jss.append(Js); Jps.append(Jd); rs.append(r); seen.extend(ids[front].tolist())
        Jf = np.concatenate(Jfs)
        ok = corners[f] >= 4 and sref._solve_spd(Jf.T @ Jf, np.zeros((6, 1)), np.float64) is not None
        status[f] = 1 if not ok else (2 if behind[f] > 0 else 0)
        out.append(dict(Jf=Jf, Js=np.concatenate(Jss), Jp=np.concatenate(Jps), r=np.concatenate(rs)))
        if ok:
            np.add.at(pcorners, np.array(seen, dtype=int), 1)
    return out, status, corners, behind, pcorners


def gauge_basis(nominal, observed):
    """Q [3 P_obs, rank] by modified Gram-Schmidt in the order translations, rotations, scale; a column is dropped at GAUGE_TOL"""
    u = nominal[observed] - nominal[observed].mean(axis=0)
    cols = [np.tile(e, len(u)) for e in np.eye(3)] + [np.cross(e, u).reshape(-1) for e in np.eye(3)] + [u.reshape(-1)]
    Q = []
    for q in cols:
        q = q.astype(np.float64).copy()
        before = np.linalg.norm(q)
        for k in Q:
            q -= (k @ q) * k
        after = np.linalg.norm(q)
        if after > GAUGE_TOL * before:
            Q.append(q / after)
    return np.stack(Q, axis=1) if Q else np.zeros((3 * len(u), 0))


def _shared_scale(frames, status):
    """c_j = 1 / sqrt(sum over usable frames of the pose-marginalised J_s^T J_s [j][j]) (1 where the sum is 0), as in 4.12"""
    D = frames[0]["Js"].shape[1]
    d = np.zeros(D)
    for fr, st in zip(frames, status):
        if st == 1:
            continue
        W = fr["Jf"].T @ fr["Js"]
        d += np.diag(fr["Js"].T @ fr["Js"] - W.T @ np.linalg.solve(fr["Jf"].T @ fr["Jf"], W))
    return np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 1.0)


def step(case, route="normal", rows=rows_analytic):
    """-> dict(refined, point_status, point_corners, frame_status, corners, behind, gauge_rank, result_status, cost, predicted_decrease, d)"""
    points, nominal, lam = np.asarray(case["points"], dtype=np.float64), np.asarray(case["nominal"], dtype=np.float64), float(case["lam"])
    frames, status, corners, behind, pcorners = frame_rows(case, rows)
    P, D = len(points), frames[0]["Js"].shape[1]
    pstat = (pcorners == 0).astype(int)
    obs = np.where(pstat == 0)[0]
    res = dict(refined=points.copy(), point_status=pstat, point_corners=pcorners, frame_status=status, corners=corners, behind=behind, gauge_rank=0,
               result_status=SINGULAR, cost=np.nan, predicted_decrease=np.nan, d=np.zeros_like(points))
    if len(obs) == 0:
        return res
    cols = (3 * obs[:, None] + np.arange(3)[None, :]).reshape(-1)
    usable = [fr for fr, st in zip(frames, status) if st != 1]
    cost = 0.5 * sum(float(fr["r"] @ fr["r"]) for fr in usable)
    Q = gauge_basis(nominal, obs)
    Pi = np.eye(len(cols)) - Q @ Q.T
    e = Pi @ (points - nominal)[obs].reshape(-1)
    cs = _shared_scale(frames, status) if D else np.zeros(0)
    n = len(cols)
    if route == "normal":
        S = np.zeros((D + n, D + n)); g = np.zeros(D + n)
        for fr in usable:
            J = np.concatenate([fr["Js"], fr["Jp"][:, cols]], axis=1)
            Hff, W = fr["Jf"].T @ fr["Jf"], fr["Jf"].T @ J
            X = np.linalg.solve(Hff, np.concatenate([W, (fr["Jf"].T @ fr["r"])[:, None]], axis=1))
            S += J.T @ J - W.T @ X[:, :-1]
            g -= J.T @ fr["r"] - W.T @ X[:, -1]
        Sdd, gd = S[D:, D:], g[D:]
        if D:
            Sss = (S[:D, :D] * cs[:, None]) * cs[None, :] + PRIOR_S * np.eye(D)
            Sds = S[D:, :D] * cs[None, :]
            X = np.linalg.solve(Sss, np.concatenate([Sds.T, (cs * g[:D])[:, None]], axis=1))
            Sdd = Sdd - Sds @ X[:, :-1]
            gd = gd - Sds @ X[:, -1]
        M = Sdd + lam * np.eye(n)
        b = gd - lam * e
        mu = np.trace(M) / n
        A = Pi @ M @ Pi + mu * (Q @ Q.T)
        A = 0.5 * (A + A.T)
        rhs = Pi @ b
        if sref._solve_spd(A, rhs[:, None].copy(), np.float64) is None:
            return res
        d = np.linalg.solve(A, rhs)
        pred = 0.5 * float(d @ rhs)
        res["pivot_margin"] = float((np.diag(np.linalg.cholesky(A)) ** 2).min() / np.diag(A).max())      # the smallest pivot over the largest diagonal entry
    else:
        nf = len(usable)

        def stack(with_target):
            nr = sum(len(fr["r"]) for fr in usable)
            width = 6 * nf + D + (n if with_target else 0)
            J = np.zeros((nr + D + n, width)); y = np.zeros(nr + D + n)
            o = 0
            for k, fr in enumerate(usable):
                m = len(fr["r"])
                J[o:o + m, 6 * k:6 * k + 6] = fr["Jf"]; J[o:o + m, 6 * nf:6 * nf + D] = fr["Js"]
                if with_target:
                    J[o:o + m, 6 * nf + D:] = fr["Jp"][:, cols] @ Pi
                y[o:o + m] = -fr["r"]
                o += m
            J[o:o + D, 6 * nf:6 * nf + D] = np.diag(np.sqrt(PRIOR_S) / cs) if D else 0.0
            o += D
            if with_target:
                J[o:, 6 * nf + D:] = np.sqrt(lam) * Pi
            y[o:] = -np.sqrt(lam) * e
            x = np.linalg.lstsq(J, y, rcond=None)[0]
            return x, 0.5 * float(np.sum((J @ x - y) ** 2))
        x, f_with = stack(True)
        _, f_without = stack(False)
        d = Pi @ x[6 * nf + D:]
        pred = f_without - f_with
    refined = points.copy()
    refined[obs] = nominal[obs] + (e + d).reshape(-1, 3)
    dd = np.zeros_like(points); dd[obs] = d.reshape(-1, 3)
    res.update(refined=refined, gauge_rank=Q.shape[1], result_status=OK, cost=cost, predicted_decrease=pred, d=dd)
    return res


def gauge_residual(case, refined, point_status):
    """|Q^T (refined - nominal)| over the observed points, the largest entry"""
    obs = np.where(np.asarray(point_status) == 0)[0]
    nominal = np.asarray(case["nominal"], dtype=np.float64)
    Q = gauge_basis(nominal, obs)
    return float(np.abs(Q.T @ (np.asarray(refined)[obs] - nominal[obs]).reshape(-1)).max()) if Q.shape[1] else 0.0
