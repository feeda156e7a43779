"""TEST INFRASTRUCTURE: the numpy reference of depth registration (include/vicalib_amd.h, vc_regist*).  Cameras go through the oracle
only -- oracle_lib.project forwards, and an inverse built on it here (the oracle's radial profile, bracketed on a grid, then Newton with
the oracle's own Jacobian inside the bracket) --, never through vc_register.hpp.  Rays, candidates, rectangles, the key minimum,
counters, visibility and the bilinear rule, all on plain arrays."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle_lib as ol          # noqa: E402
from vicalib_amd import synth    # noqa: E402

KIND_Z, KIND_RANGE = 0, 1
NEAREST, FOOTPRINT = 0, 1
MAX_FOOTPRINT = 8
BORDER_TOL = 1e-9                 # the undistorter's border rule
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
KB4 = synth.MODEL_IDS["kb4"]


def _mid(model):
    return synth.MODEL_IDS[model] if isinstance(model, str) else int(model)


def project(model, K, pts):
    """oracle_lib.project of every point [n, 3] -> [n, 2] (NaN where the oracle gives none)"""
    m = _mid(model)
    K = np.ascontiguousarray(K, dtype=np.float64)
    pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, 3))
    out = np.empty((len(pts), 2))
    with np.errstate(all="ignore"):
        for k in range(len(pts)):
            out[k] = ol.project(m, pts[k], K)[0]
    return out


def _profile(model, Kn, t):
    """(f, f') of the radial profile at unit focal length, from the oracle's projection and its Jacobian with respect to the ray"""
    m = _mid(model)
    f = np.empty(len(t)); df = np.empty(len(t))
    for k, tk in enumerate(t):
        ray = np.array([np.sin(tk), 0.0, np.cos(tk)]) if m == KB4 else np.array([tk, 0.0, 1.0])
        pix, dray, _ = ol.project(m, ray, Kn)
        f[k] = pix[0]
        df[k] = dray[0, 0] * ray[2] - dray[0, 2] * ray[0] if m == KB4 else dray[0, 0]
    return f, df


def unproject(model, K, px, peak_margin=1e-4):
    """rays [n, 3] of the pixels px [n, 2] and has_ray [n]: the smallest t with profile(t) = r_d on the profile's first increasing branch.
    A pixel beyond the branch's maximum has no ray.  Asserts that no pixel lies within peak_margin of that maximum (where an iterative
    inverse may or may not converge): a condition on the case."""
    m = _mid(model)
    K = np.asarray(K, dtype=np.float64)
    Kn = np.concatenate([[1.0, 1.0, 0.0, 0.0], K[4:]])
    px = np.asarray(px, dtype=np.float64).reshape(-1, 2)
    d = (px - K[2:4]) / K[:2]
    rd = np.hypot(d[:, 0], d[:, 1]); phi = np.arctan2(d[:, 1], d[:, 0])
    grid = np.linspace(0.0, 3.1 if m == KB4 else 6.0, 1201)
    fg, _ = _profile(m, Kn, grid)
    rising = np.diff(fg) > 0
    last = len(grid) - 1 if rising.all() else int(np.argmin(rising))          # the grid's maximum of the first branch
    peak = fg[last]
    assert np.all(np.abs(rd - peak) > peak_margin), "a pixel at the edge of the model's image"
    has = rd < peak
    t = np.zeros(len(rd))
    idx = np.nonzero(has & (rd > 0))[0]
    hi_i = np.searchsorted(fg[:last + 1], rd[idx], side="left")                # fg[hi_i - 1] < rd <= fg[hi_i]
    lo, hi = grid[hi_i - 1], grid[hi_i]
    x = 0.5 * (lo + hi)
    for _ in range(60):
        f, df = _profile(m, Kn, x)
        res = f - rd[idx]
        hi = np.where(res > 0, x, hi); lo = np.where(res <= 0, x, lo)
        done = np.abs(res) <= 1e-15 * (1.0 + rd[idx])
        if done.all():
            break
        with np.errstate(all="ignore"):
            nx = x - res / df
        bad = ~(nx > lo) | ~(nx < hi)                                          # a step out of the bracket: bisect
        nx = np.where(bad, 0.5 * (lo + hi), nx)
        moved = nx != x
        x = np.where(done, x, nx)
        if not (moved & ~done).any():
            break
    t[idx] = x
    c, s = np.cos(phi), np.sin(phi)
    if m == KB4:
        rays = np.stack([np.sin(t) * c, np.sin(t) * s, np.cos(t)], axis=-1)
    else:
        rays = np.stack([t * c, t * s, np.ones_like(t)], axis=-1)
    rays[~has] = np.nan
    return rays, has


def quat_matrix(q):
    x, y, z, w = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def relative_pose(T_ck_s, T_ck_d):
    """p_d = R p_s + t from p_c = R_ck p_k + t_ck"""
    Rs, Rd = quat_matrix(T_ck_s[:4]), quat_matrix(T_ck_d[:4])
    R = Rd @ Rs.T
    return R, np.asarray(T_ck_d[4:], dtype=np.float64) - R @ np.asarray(T_ck_s[4:], dtype=np.float64)


class Setup:
    """Two cameras (model, K, (w, h), T_ck), units, kind, splat: what a registrar is made of"""

    def __init__(self, cam_s, cam_d, unit_src, unit_dst, kind, splat):
        self.cam_s, self.cam_d = cam_s, cam_d
        self.unit_src, self.unit_dst, self.kind, self.splat = float(unit_src), float(unit_dst), int(kind), int(splat)
        self.R, self.t = relative_pose(cam_s[3], cam_d[3])

    def transfer(self, rays, m):
        """points at measured distance m [n] on rays [n, 3] -> (q [n, 2], value in D's unit [n], in front / finite [n])"""
        rays = np.asarray(rays, dtype=np.float64); m = np.asarray(m, dtype=np.float64)
        with np.errstate(all="ignore"):
            s = m / rays[:, 2] if self.kind == KIND_Z else m / np.linalg.norm(rays, axis=1)
            pd = (rays * s[:, None]) @ self.R.T + self.t
            ok = np.isfinite(pd).all(axis=1)
            front = ok & ((pd[:, 2] > 0.0) | (_mid(self.cam_d[0]) == KB4))
            q = np.full((len(pd), 2), np.nan)
            q[front] = project(self.cam_d[0], self.cam_d[1], pd[front])
            front &= np.isfinite(q).all(axis=1)
            wv = (pd[:, 2] if self.kind == KIND_Z else np.linalg.norm(pd, axis=1)) / self.unit_dst
        return q, wv, front, pd[:, 2]

    def rays(self, px):
        rays, has = unproject(self.cam_s[0], self.cam_s[1], px)
        if self.kind == KIND_Z:
            with np.errstate(invalid="ignore"):
                has = has & (rays[:, 2] > 0.0)
        return rays, has

    def points(self, rows):
        """the continuous face of rows (u, v, value) -> ((q_x, q_y, m_d / unit_dst) [n, 3], valid [n])"""
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
        rays, has = self.rays(rows[:, :2])
        out = np.full((len(rows), 3), np.nan)
        q, wv, front, _ = self.transfer(rays[has], rows[has, 2] * self.unit_src)
        sel = np.nonzero(has)[0][front]
        out[sel, :2] = q[front]; out[sel, 2] = wv[front]
        return out, ~np.isnan(out[:, 0])


class Tables:
    """rays of the pixel centres and of the corner lattice of the source camera (they depend on the source camera and the kind only)"""

    def __init__(self, setup):
        w, h = setup.cam_s[2]
        jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        self.centre, self.centre_ok = setup.rays(np.stack([ii.ravel(), jj.ravel()], axis=-1).astype(np.float64))
        jj, ii = np.meshgrid(np.arange(h + 1), np.arange(w + 1), indexing="ij")
        lat, lat_ok = setup.rays(np.stack([ii.ravel() - 0.5, jj.ravel() - 0.5], axis=-1))
        lat = lat.reshape(h + 1, w + 1, 3); lat_ok = lat_ok.reshape(h + 1, w + 1)
        self.a, self.a_ok = lat[:-1, :-1].reshape(-1, 3), lat_ok[:-1, :-1].ravel()          # (i - 0.5, j - 0.5)
        self.b, self.b_ok = lat[1:, 1:].reshape(-1, 3), lat_ok[1:, 1:].ravel()              # (i + 0.5, j + 0.5)


def depth_test(setup, tables, depth):
    """One depth image [h_s, w_s] uint16 through the definitions.  Returns a dict: per source pixel `code` (the rule that dropped it, 6 =
    candidate), q, wv, z_d and -- what the rounding acts on -- `edges` [n, 4] = x0, x1, y0, y1 before the floor and `warg` = wv + 0.5;
    per destination pixel `depth`, `index`, `hits` (candidates landed), `distinct` (different w among them), `ties` (the winning w landed
    from more than one source pixel); `counters` [8]."""
    ws, hs = setup.cam_s[2]; wd, hd = setup.cam_d[2]
    v = np.asarray(depth).reshape(-1).astype(np.int64)
    n = len(v)
    fp = setup.splat == FOOTPRINT
    code = np.full(n, -1)
    code[v == 0] = 0
    has = tables.centre_ok & ((tables.a_ok & tables.b_ok) if fp else True)
    code[(code < 0) & ~has] = 1
    live = np.nonzero(code < 0)[0]
    m = v[live] * setup.unit_src
    q = np.full((n, 2), np.nan); wv = np.full(n, np.nan); zd = np.full(n, np.nan)
    qc, wc, fc, zc = setup.transfer(tables.centre[live], m)
    q[live], wv[live], zd[live] = qc, wc, zc
    front = fc
    edges = np.full((n, 4), np.nan)
    if fp:
        qa, _, fa, za = setup.transfer(tables.a[live], m)
        qb, _, fb, zb = setup.transfer(tables.b[live], m)
        front = fc & fa & fb
        zd[live] = np.where(np.abs(za) < np.abs(zd[live]), za, zd[live]); zd[live] = np.where(np.abs(zb) < np.abs(zd[live]), zb, zd[live])
        edges[live] = np.stack([np.minimum(qa[:, 0], qb[:, 0]), np.maximum(qa[:, 0], qb[:, 0]), np.minimum(qa[:, 1], qb[:, 1]), np.maximum(qa[:, 1], qb[:, 1])], axis=-1) + 0.5
    else:
        edges[live] = np.stack([qc[:, 0], qc[:, 0], qc[:, 1], qc[:, 1]], axis=-1) + 0.5
    code[live[~front]] = 2
    live = live[front]
    with np.errstate(invalid="ignore"):
        r = np.floor(edges)
        outside = ~((r[:, 1] >= 0) & (r[:, 0] <= wd - 1) & (r[:, 3] >= 0) & (r[:, 2] <= hd - 1))
        wr = np.floor(wv + 0.5)
        badw = ~((wr >= 1) & (wr <= 65535))
        big = (r[:, 1] - r[:, 0] + 1 > MAX_FOOTPRINT) | (r[:, 3] - r[:, 2] + 1 > MAX_FOOTPRINT) if fp else np.zeros(n, dtype=bool)
    for rule, hit in ((3, outside), (4, badw), (5, big)):
        sel = live[hit[live]]
        code[sel] = rule
        live = live[~hit[live]]
    code[live] = 6
    keys = np.full(hd * wd, EMPTY, dtype=np.uint64)
    hits = np.zeros(hd * wd, dtype=np.int64)
    landed = [[] for _ in range(hd * wd)]
    for e in live:
        x0, x1 = int(max(r[e, 0], 0)), int(min(r[e, 1], wd - 1)); y0, y1 = int(max(r[e, 2], 0)), int(min(r[e, 3], hd - 1))
        key = (np.uint64(int(wr[e])) << np.uint64(32)) | np.uint64(int(e))
        for y in range(y0, y1 + 1):
            for x in range(x0, x1 + 1):
                p = y * wd + x
                keys[p] = min(keys[p], key); hits[p] += 1; landed[p].append(int(wr[e]))
    filled = keys != EMPTY
    out_depth = np.where(filled, keys >> np.uint64(32), 0).astype(np.uint16).reshape(hd, wd)
    out_index = np.where(filled, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32).reshape(hd, wd)
    distinct = np.array([len(set(L)) > 1 for L in landed]).reshape(hd, wd)
    ties = np.array([len(L) > 0 and L.count(min(L)) > 1 for L in landed]).reshape(hd, wd)
    counters = np.array([np.count_nonzero(code == k) for k in range(7)] + [int(filled.sum())], dtype=np.int64)
    return dict(code=code, q=q, wv=wv, z_d=zd, edges=edges, warg=wv + 0.5, depth=out_depth, index=out_index, hits=hits.reshape(hd, wd), distinct=distinct,
                ties=ties, counters=counters, keys=keys)


def bilinear(img, x, y):
    """the bilinear rule of vc_undistort_images at (x, y) inside the image, unrounded"""
    h, w = img.shape
    x0 = np.minimum(np.floor(x), w - 2).astype(int); y0 = np.minimum(np.floor(y), h - 2).astype(int)
    ax, ay = x - x0, y - y0
    p = img.astype(np.float64)
    return (1 - ay) * ((1 - ax) * p[y0, x0] + ax * p[y0, x0 + 1]) + ay * ((1 - ax) * p[y0 + 1, x0] + ax * p[y0 + 1, x0 + 1])


def gather(setup, tables, depth, test, color, occl_tol, fill):
    """Colour into depth geometry, with depth_test's result `test` of the same image.  Rules 0-2 are taken at the pixel centre.  Returns a
    dict per source pixel: `visible`, `value` (the unrounded bilinear value, NaN where not visible), `out` (uint8), `inside_by` (distance
    of q to the image border, positive inside), `lookup` (the destination pixel whose depth test decides, -1 without one), `margin` =
    w_win + occl_tol - w, and q, warg = m_d / unit_dst + 0.5 of the centre."""
    ws, hs = setup.cam_s[2]; wd, hd = setup.cam_d[2]
    v = np.asarray(depth).reshape(-1).astype(np.int64)
    n = ws * hs
    live = np.nonzero((v != 0) & tables.centre_ok)[0]
    q = np.full((n, 2), np.nan); wv = np.full(n, np.nan)
    qc, wc, fc, _ = setup.transfer(tables.centre[live], v[live] * setup.unit_src)
    q[live[fc]] = qc[fc]; wv[live[fc]] = wc[fc]
    passed = np.isfinite(q).all(axis=1)
    with np.errstate(invalid="ignore"):
        inside_by = np.minimum(np.minimum(q[:, 0], wd - 1.0 - q[:, 0]), np.minimum(q[:, 1], hd - 1.0 - q[:, 1]))
        inside = passed & (inside_by >= -BORDER_TOL)
    x = np.clip(np.where(inside, q[:, 0], 0.0), 0.0, wd - 1.0); y = np.clip(np.where(inside, q[:, 1], 0.0), 0.0, hd - 1.0)
    lookup = np.where(inside, np.floor(y + 0.5).astype(int) * wd + np.floor(x + 0.5).astype(int), -1)
    key = test["keys"][np.maximum(lookup, 0)]
    w_win = (key >> np.uint64(32)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        margin = np.where(inside & (key != EMPTY), w_win + occl_tol - np.floor(wv + 0.5), -np.inf)
    visible = margin >= 0
    value = np.where(visible, bilinear(np.asarray(color), x, y), np.nan)
    out = np.where(visible, np.floor(np.nan_to_num(value) + 0.5), fill).astype(np.uint8)
    return dict(visible=visible.reshape(hs, ws), value=value.reshape(hs, ws), out=out.reshape(hs, ws), inside_by=np.where(passed, inside_by, np.nan),
                lookup=lookup, margin=margin, passed=passed, q=q, warg=wv + 0.5)
