"""TEST INFRASTRUCTURE: the rig seed (vc_seed_rig) restated in numpy, sharing no code with vicalib_amd/csrc/vc_seed_rig.hpp: the candidates
X_k = T_aw(k) T_bw(k)^-1 of every pair with 4 x 4 matrices, the vote as a plain O(N^2) table, the refit's sums with math.fsum, the tree and
its poses with 4 x 4 matrices.  Besides what the library returns it reports `margin`: the smallest relative distance of any comparison of
the vote from either of its two thresholds, which tests/seed_rig_cases.py holds above 1e-9 so that a difference in contraction between two
builds cannot flip a vote."""
import math

import numpy as np


def quat_to_matrix(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def matrix_to_quat(R):
    """[x y z w], w >= 0 (Shepperd's branches)"""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0.0:
        s = 2.0 * math.sqrt(tr + 1.0); q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = 2.0 * math.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]); q = [0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s]
    elif R[1, 1] > R[2, 2]:
        s = 2.0 * math.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]); q = [(R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s]
    else:
        s = 2.0 * math.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]); q = [(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s, (R[1, 0] - R[0, 1]) / s]
    q = np.array(q)
    q /= np.linalg.norm(q)
    return -q if q[3] < 0.0 else q


def pose_to_matrix(T):
    M = np.eye(4); M[:3, :3] = quat_to_matrix(np.asarray(T[:4], dtype=np.float64)); M[:3, 3] = T[4:7]
    return M


def matrix_to_pose(M):
    return np.concatenate([matrix_to_quat(M[:3, :3]), M[:3, 3]])


def quat_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def pair_order(n_cams):
    return [(a, b) for a in range(n_cams) for b in range(a + 1, n_cams)]


def candidates(Ta, Tb):
    """q [n, 4] (unit; the quaternion product, so that a negated input quaternion negates it), t [n, 3], d [n] of X = T_a T_b^-1"""
    n = len(Ta)
    q = np.zeros((n, 4)); t = np.zeros((n, 3)); d = np.zeros(n)
    for k in range(n):
        qa, qb = Ta[k, :4], Tb[k, :4]
        q[k] = quat_mul(qa, qb * np.array([-1.0, -1.0, -1.0, 1.0]))
        q[k] /= np.linalg.norm(q[k])
        X = pose_to_matrix(Ta[k]) @ np.linalg.inv(pose_to_matrix(Tb[k]))
        t[k] = X[:3, 3]
        d[k] = max(np.linalg.norm(Ta[k, 4:]), np.linalg.norm(Tb[k, 4:]))
    return q, t, d


def vote(q, t, d, tol_deg):
    """agree [n, n] and the smallest relative distance of a comparison from its threshold"""
    tol = math.radians(tol_deg)
    c = math.cos(0.5 * tol)
    dot = np.abs(q @ q.T)
    dt2 = ((t[:, None, :] - t[None, :, :]) ** 2).sum(axis=2)
    thr = tol * tol * (d[:, None] + d[None, :]) ** 2
    margin = min(np.min(np.abs(dot - c) / c), np.min(np.abs(dt2 - thr) / thr)) if len(q) else np.inf
    return (dot >= c) & (dt2 <= thr), float(margin)


def pair(view_ok, view_T, a, b, tol_deg, min_support):
    frames = np.nonzero((view_ok[:, a] != 0) & (view_ok[:, b] != 0))[0]
    r = dict(shared=len(frames), status=0, margin=np.inf)
    if len(frames) == 0:
        r["status"] = 1
        return r
    q, t, d = candidates(view_T[frames, a], view_T[frames, b])
    agree, r["margin"] = vote(q, t, d, tol_deg)
    support = agree.sum(axis=1)
    w = int(np.argmax(support))                      # (the first of equals)
    r["all_support"] = support; r["frames"] = frames
    if support[w] < min_support:
        r["status"] = 2
        return r
    members = np.nonzero(agree[w])[0]
    s = np.where(q[members] @ q[w] < 0.0, -1.0, 1.0)
    qs = np.array([math.fsum(s * q[members, k]) for k in range(4)])
    qs /= math.sqrt(math.fsum(qs * qs))
    if qs[3] < 0.0:
        qs = -qs
    tm = np.array([math.fsum(t[members, k]) for k in range(3)]) / len(members)
    ang2, dist2 = [], []
    for j in members:
        rel = quat_mul(qs * np.array([-1.0, -1.0, -1.0, 1.0]), q[j])
        ang2.append((2.0 * math.atan2(math.sqrt(math.fsum(rel[:3] ** 2)), abs(rel[3]))) ** 2)
        dist2.append(math.fsum((t[j] - tm) ** 2))
    r.update(support=int(support[w]), winner=int(frames[w]), T_ab=np.concatenate([qs, tm]), rms_deg=math.degrees(math.sqrt(math.fsum(ang2) / len(members))),
             rms_m=math.sqrt(math.fsum(dist2) / len(members)), members=frames[members])
    return r


def tree(n_cams, pairs):
    """Prim from camera 0 over the status-0 pairs by support; ties: the lowest tree camera, then the lowest new camera"""
    order = pair_order(n_cams)
    edge = {ab: pairs[p] for p, ab in enumerate(order) if pairs[p]["status"] == 0}
    parent = [-1] * n_cams; status = [1] * n_cams; M = [None] * n_cams
    status[0] = 0; M[0] = np.eye(4)
    while True:
        best = None
        for u in [c for c in range(n_cams) if status[c] == 0]:
            for v in [c for c in range(n_cams) if status[c] == 1]:
                e = edge.get((min(u, v), max(u, v)))
                if e is not None and (best is None or e["support"] > best[0]):
                    best = (e["support"], u, v)
        if best is None:
            break
        _, u, v = best
        X = pose_to_matrix(edge[(min(u, v), max(u, v))]["T_ab"])          # the higher camera into the lower
        M[v] = (np.linalg.inv(X) if u < v else X) @ M[u]
        parent[v] = u; status[v] = 0
    return parent, status, M


def seed(view_ok, view_T, tol_deg=3.0, min_support=3):
    """what vicalib_amd.lib.seed_rig returns, with None / NaN where the library leaves its output untouched, the per-pair records (`pairs`) and `margin`"""
    view_ok = np.asarray(view_ok); view_T = np.asarray(view_T, dtype=np.float64)
    n_cams = view_ok.shape[1]
    order = pair_order(n_cams)
    pairs = [pair(view_ok, view_T, a, b, tol_deg, min_support) for a, b in order]
    P = len(order)
    r = dict(pair_T_ab=np.full((P, 7), np.nan), pair_shared=np.array([p["shared"] for p in pairs], dtype=np.int32), pair_support=np.full(P, -1, dtype=np.int32),
             pair_winner=np.full(P, -1, dtype=np.int32), pair_rms_deg=np.full(P, np.nan), pair_rms_m=np.full(P, np.nan),
             pair_status=np.array([p["status"] for p in pairs], dtype=np.int32), pairs=pairs, margin=min([p["margin"] for p in pairs] + [np.inf]))
    for i, p in enumerate(pairs):
        if p["status"] == 0:
            r["pair_T_ab"][i] = p["T_ab"]; r["pair_support"][i] = p["support"]; r["pair_winner"][i] = p["winner"]
            r["pair_rms_deg"][i] = p["rms_deg"]; r["pair_rms_m"][i] = p["rms_m"]
    parent, status, M = tree(n_cams, pairs)
    r["cam_parent"] = np.array(parent, dtype=np.int32); r["cam_status"] = np.array(status, dtype=np.int32)
    r["cam_T_c0"] = np.array([matrix_to_pose(M[c]) if status[c] == 0 else np.full(7, np.nan) for c in range(n_cams)])
    return r
