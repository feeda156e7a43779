"""The focal-length seed (vc_seed_focal_batch, vicalib_amd/csrc/vc_seed_focal.hpp) restated in numpy: the reference of tests/seed_focal_cases.py.

Per view, with the camera's principal point (cx, cy) and a radius R in pixels:
  used corner   both coordinates finite and (u - cx)^2 + (v - cy)^2 <= R^2; R <= 0: every finite corner
  status 1      fewer than max(min_corners, 4) used corners
  status 2      a used target point more than 1e-9 off the plane z = z of the first used corner
  H             normalised DLT from target (X, Y) to (u - cx, v - cy): Hartley normalisation of both sides (centroid, mean distance sqrt 2),
                the eigenvector of the smallest eigenvalue of A^T A (route "eigh": numpy.linalg.eigh on the 9 x 9 matrix; route "svd":
                numpy.linalg.svd of the unsquared 2m x 9 matrix A), de-normalised.  status 3 when that fails or H is not finite
  fit_px        rms transfer error of H over the used corners; status 4 when max_fit_px > 0 and fit_px > max_fit_px
  scaling       h1x^2 + h1y^2 + h2x^2 + h2y^2 = 2 for the first two columns h1, h2 of H
  rows          c1 = h1x h2x + h1y h2y, d1 = -h1z h2z, c2 = (h1x^2 + h1y^2) - (h2x^2 + h2y^2), d2 = h2z^2 - h1z^2
  view_f        1 / sqrt((c1 d1 + c2 d2) / (c1^2 + c2^2)); NaN when the quotient is not positive or c1^2 + c2^2 < sin^4(min_tilt)
Per camera, over its status-0 views in view order: Scc = sum(c1^2 + c2^2), Scd = sum(c1 d1 + c2 d2); status 1 no usable view, 2 Scc <
sin^4(min_tilt), 3 Scd / Scc not positive or not finite; otherwise f = sqrt(Scc / Scd)."""
import numpy as np

OK, FEW, NOT_PLANAR, NO_H, BAD_FIT = range(5)
CAM_OK, CAM_NO_VIEW, CAM_NO_TILT, CAM_NO_FOCAL = range(4)


def sin4(min_tilt_deg):
    return float(np.sin(np.deg2rad(min_tilt_deg)) ** 4)


def dlt(XY, xy, route):
    """H with (x, y, 1) ~ H (X, Y, 1), or None"""
    m = len(XY)
    mW, mI = XY.mean(axis=0), xy.mean(axis=0)
    dW, dI = np.linalg.norm(XY - mW, axis=1).sum(), np.linalg.norm(xy - mI, axis=1).sum()
    if not (dW > 0 and dI > 0):
        return None
    sW, sI = np.sqrt(2.0) * m / dW, np.sqrt(2.0) * m / dI
    P, p = (XY - mW) * sW, (xy - mI) * sI
    A = np.zeros((2 * m, 9))
    A[0::2, 0], A[0::2, 1], A[0::2, 2] = -P[:, 0], -P[:, 1], -1.0
    A[0::2, 6], A[0::2, 7], A[0::2, 8] = p[:, 0] * P[:, 0], p[:, 0] * P[:, 1], p[:, 0]
    A[1::2, 3], A[1::2, 4], A[1::2, 5] = -P[:, 0], -P[:, 1], -1.0
    A[1::2, 6], A[1::2, 7], A[1::2, 8] = p[:, 1] * P[:, 0], p[:, 1] * P[:, 1], p[:, 1]
    try:
        if route == "eigh":
            Hn = np.linalg.eigh(A.T @ A)[1][:, 0]
        else:
            Hn = np.linalg.svd(A, full_matrices=True)[2][-1]
    except np.linalg.LinAlgError:
        return None
    Tw = np.array([[sW, 0, -sW * mW[0]], [0, sW, -sW * mW[1]], [0, 0, 1.0]])
    TiInv = np.array([[1 / sI, 0, mI[0]], [0, 1 / sI, mI[1]], [0, 0, 1.0]])
    return TiInv @ Hn.reshape(3, 3) @ Tw


def view(pw, uv, cx, cy, R, min_corners=4, max_fit_px=0.0, min_tilt_deg=5.0, route="eigh"):
    """dict(status, and with status 0: H [3, 3], rows [4], f, fit_px, used)"""
    pw, uv = np.asarray(pw, dtype=np.float64).reshape(-1, 3), np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        xy = uv - np.array([cx, cy])
        use = np.isfinite(uv).all(axis=1)
        if R > 0:
            use &= (xy ** 2).sum(axis=1) <= R * R
    m = int(use.sum())
    if m < max(int(min_corners), 4):
        return dict(status=FEW)
    P, p = pw[use], xy[use]
    if not np.all(np.abs(P[:, 2] - P[0, 2]) <= 1e-9):
        return dict(status=NOT_PLANAR)
    H = dlt(P[:, :2], p, route)
    if H is None or not np.isfinite(H).all():
        return dict(status=NO_H)
    with np.errstate(all="ignore"):
        q = np.concatenate([P[:, :2], np.ones((m, 1))], axis=1) @ H.T
        fit = float(np.sqrt((((q[:, :2] / q[:, 2:3]) - p) ** 2).sum() / m))
        if max_fit_px > 0 and not fit <= max_fit_px:
            return dict(status=BAD_FIT)
        H = H * np.sqrt(2.0 / (H[0, 0] ** 2 + H[1, 0] ** 2 + H[0, 1] ** 2 + H[1, 1] ** 2))
        if not np.isfinite(H).all():
            return dict(status=NO_H)
        h1, h2 = H[:, 0], H[:, 1]
        c1, d1 = h1[0] * h2[0] + h1[1] * h2[1], -h1[2] * h2[2]
        c2, d2 = (h1[0] ** 2 + h1[1] ** 2) - (h2[0] ** 2 + h2[1] ** 2), h2[2] ** 2 - h1[2] ** 2
        cc = c1 * c1 + c2 * c2
        quot = (c1 * d1 + c2 * d2) / cc
        f = 1.0 / np.sqrt(quot) if (quot > 0 and cc >= sin4(min_tilt_deg)) else np.nan
    return dict(status=OK, H=H, rows=np.array([c1, d1, c2, d2]), f=float(f), fit_px=fit, used=m)


def batch(view_cam, cam_pp, cam_radius, view_off, p_w, p_c, min_corners=4, max_fit_px=0.0, min_tilt_deg=5.0, route="eigh"):
    """the layout of vicalib_amd.lib.seed_focal_batch; NaN (0 for view_used) where a view or a camera is refused"""
    n, nc = len(view_cam), len(cam_radius)
    cam_pp = np.asarray(cam_pp, dtype=np.float64).reshape(-1, 2)
    out = dict(view_H=np.full((n, 3, 3), np.nan), view_rows=np.full((n, 4), np.nan), view_f=np.full(n, np.nan), view_fit_px=np.full(n, np.nan),
               view_used=np.zeros(n, dtype=np.int32), view_status=np.zeros(n, dtype=np.int32), cam_f=np.full(nc, np.nan),
               cam_views=np.zeros(nc, dtype=np.int32), cam_status=np.zeros(nc, dtype=np.int32))
    for v in range(n):
        c = int(view_cam[v])
        r = view(p_w[view_off[v]:view_off[v + 1]], p_c[view_off[v]:view_off[v + 1]], cam_pp[c, 0], cam_pp[c, 1], cam_radius[c], min_corners, max_fit_px,
                 min_tilt_deg, route)
        out["view_status"][v] = r["status"]
        if r["status"] == OK:
            out["view_H"][v], out["view_rows"][v], out["view_f"][v], out["view_fit_px"][v], out["view_used"][v] = r["H"], r["rows"], r["f"], r["fit_px"], r["used"]
    for c in range(nc):
        scc = scd = 0.0
        cnt = 0
        for v in range(n):                                       # fixed order: view order
            if int(view_cam[v]) == c and out["view_status"][v] == OK:
                c1, d1, c2, d2 = out["view_rows"][v]
                scc += c1 * c1 + c2 * c2; scd += c1 * d1 + c2 * d2; cnt += 1
        out["cam_views"][c] = cnt
        if cnt == 0:
            out["cam_status"][c] = CAM_NO_VIEW
        elif not scc >= sin4(min_tilt_deg):
            out["cam_status"][c] = CAM_NO_TILT
        elif not (scd / scc > 0 and np.isfinite(scd / scc)):
            out["cam_status"][c] = CAM_NO_FOCAL
        else:
            out["cam_f"][c] = np.sqrt(scc / scd)
    return out
