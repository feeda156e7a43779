"""TEST INFRASTRUCTURE: the numpy reference of the depth calibration (include/vicalib_amd.h, vc_depthcal*).  Rays come from
register_ref.unproject (the oracle's projection, inverted there) and rotations from register_ref.quat_matrix, never from
vc_depthcal.hpp; the rules, the sums (in extended precision), the fit and the correction are restated here on plain arrays."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import register_ref as rr        # noqa: E402

KIND_Z, KIND_RANGE = rr.KIND_Z, rr.KIND_RANGE
CELL, BILINEAR = 0, 1
EPS = float(np.finfo(np.float64).eps)


class Setup:
    """What a depth calibrator is made of: cam = (model, K, (w, h), T_ck)"""

    def __init__(self, cam, rect, bins, unit, kind, v_ref, min_cos, max_dev):
        self.cam, self.rect, self.bins = cam, tuple(float(x) for x in rect), (int(bins[0]), int(bins[1]))
        self.unit, self.kind, self.v_ref, self.min_cos, self.max_dev = float(unit), int(kind), float(v_ref), float(min_cos), float(max_dev)
        self.size = tuple(cam[2])
        self.cells = self.bins[0] * self.bins[1]

    def rays(self):
        """(rays [h w, 3], has_ray [h w]) of the pixel centres: the registrar's rule 1"""
        w, h = self.size
        jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        rays, has = rr.unproject(self.cam[0], self.cam[1], np.stack([ii.ravel(), jj.ravel()], axis=-1).astype(np.float64))
        if self.kind == KIND_Z:
            with np.errstate(invalid="ignore"):
                has = has & (rays[:, 2] > 0.0)
        return rays, has

    def cell_map(self):
        """[h, w] the cell index cy * bins_x + cx of every pixel (the binning of the report's error maps)"""
        w, h = self.size
        cx = np.clip(np.floor(np.arange(w) * float(self.bins[0]) / float(w)), 0, self.bins[0] - 1).astype(int)
        cy = np.clip(np.floor(np.arange(h) * float(self.bins[1]) / float(h)), 0, self.bins[1] - 1).astype(int)
        return cy[:, None] * self.bins[0] + cx[None, :]


def frame(T_ck, T_wk):
    """R_wc, c_w from p_c = R_ck p_k + t_ck and p_w = R_wk p_k + t_wk"""
    R_ck, R_wk = rr.quat_matrix(T_ck[:4]), rr.quat_matrix(T_wk[:4])
    R_wc = R_wk @ R_ck.T
    return R_wc, np.asarray(T_wk[4:], dtype=np.float64) - R_wc @ np.asarray(T_ck[4:], dtype=np.float64)


def expected(setup, rays, has, T_wk, depth=None):
    """One frame through the definitions -> dict per pixel [h w]: y (NaN under rules 1 and 2), rule, and what the thresholds act on:
    `edge` (distance of the hit to the rectangle's border, positive inside), `cosm` (|d_w.z| / |d_w| - min_cos), `s`."""
    n = len(rays)
    R_wc, c_w = frame(setup.cam[3], T_wk)
    with np.errstate(all="ignore"):
        d_w = rays @ R_wc.T
        s = -c_w[2] / d_w[:, 2]
        front = has & np.isfinite(s) & (s > 0)
        hit = c_w[None, :] + s[:, None] * d_w
        e = s * (rays[:, 2] if setup.kind == KIND_Z else np.linalg.norm(rays, axis=1))
        y = np.where(front, e / setup.unit, np.nan)
        x0, y0, x1, y1 = setup.rect
        edge = np.minimum(np.minimum(hit[:, 0] - x0, x1 - hit[:, 0]), np.minimum(hit[:, 1] - y0, y1 - hit[:, 1]))
        cosm = np.abs(d_w[:, 2]) / np.linalg.norm(d_w, axis=1) - setup.min_cos
        rule = np.full(n, 7)
        v = None if depth is None else np.asarray(depth).reshape(-1).astype(np.float64)
        if v is not None:
            rule[np.abs(y - v) > setup.max_dev] = 6
        rule[~((y >= 1.0) & (y <= 65535.0))] = 5
        rule[cosm < 0] = 4
        rule[~(edge >= 0)] = 3
        rule[~front] = 2
        rule[~has] = 1
        if v is not None:
            rule[v == 0] = 0
    return dict(y=y, rule=rule, edge=np.where(front, edge, np.nan), cosm=np.where(front, cosm, np.nan), s=s)


def terms(setup, v, y):
    """[n, 9] the terms of used pixels with values v and expected values y, in extended precision"""
    v = np.asarray(v, dtype=np.longdouble); y = np.asarray(y, dtype=np.longdouble)
    x = (v - setup.v_ref) / setup.v_ref
    d = y - v
    return np.stack([np.ones_like(x), x, x * x, x ** 3, x ** 4, d, d * x, d * x * x, d * d], axis=-1)


def accumulate(setup, rays, has, depth, poses, d_y):
    """The sums of the frames `depth` [n, h, w] at `poses` [n, 7] -> dict(sums [cells, 9] float64 (summed in extended precision), counters
    [n, 8], bound [cells, 9], rules [n, h w], y [n, h w]).  The bound on a sum is derived: sum |dt/dy| d_y over its terms (t depends
    on y through d = y - v only) plus n_terms eps sum |t| for any order of summation."""
    cells = setup.cell_map().ravel()
    sums = np.zeros((setup.cells, 9), dtype=np.longdouble); bound = np.zeros((setup.cells, 9)); absum = np.zeros((setup.cells, 9)); count = np.zeros(setup.cells)
    counters = np.zeros((len(depth), 8), dtype=np.int64)
    rules, ys = [], []
    for k, (img, T) in enumerate(zip(depth, poses)):
        ex = expected(setup, rays, has, T, img)
        rules.append(ex["rule"]); ys.append(ex["y"])
        counters[k] = np.bincount(ex["rule"], minlength=8)
        used = ex["rule"] == 7
        v = np.asarray(img).reshape(-1)[used]
        t = terms(setup, v, ex["y"][used])
        x = np.abs(np.asarray(t[:, 1], dtype=np.float64)); d = np.abs(np.asarray(t[:, 5], dtype=np.float64))
        dtdy = np.stack([0 * x, 0 * x, 0 * x, 0 * x, 0 * x, 1 + 0 * x, x, x * x, 2 * d], axis=-1)
        for c in range(setup.cells):
            m = cells[used] == c
            sums[c] += t[m].sum(axis=0)
            bound[c] += dtdy[m].sum(axis=0) * d_y
            absum[c] += np.abs(np.asarray(t[m], dtype=np.float64)).sum(axis=0)
            count[c] += m.sum()
    bound += (count[:, None] + 4.0) * EPS * absum           # (+ 4: the roundings inside a term itself)
    return dict(sums=np.asarray(sums, dtype=np.float64), counters=counters, bound=bound, rules=np.stack(rules), y=np.stack(ys))


def fit(sums, degree, min_count, min_spread):
    """The two-stage fit of sums [cells, 9] -> dict(c [3], a, b, status [cells], rms [3]); None without a pixel or with a singular system.
    Stage 1 through numpy's solver, stage 2 as centred regressions: another arrangement of the algebra than the library's."""
    S = np.asarray(sums, dtype=np.float64)
    T = S.sum(axis=0)
    if not T[0] >= 1:
        return None
    m = degree + 1
    M = np.array([[T[i + j] for j in range(m)] for i in range(m)])
    try:
        if np.any(np.linalg.eigvalsh(M) <= 0):
            return None
        c = np.zeros(3); c[:m] = np.linalg.solve(M, T[5:5 + m])
    except np.linalg.LinAlgError:
        return None

    def remainder(S):
        Sr = S[..., 5] - (c[0] * S[..., 0] + c[1] * S[..., 1] + c[2] * S[..., 2])
        Srx = S[..., 6] - (c[0] * S[..., 1] + c[1] * S[..., 2] + c[2] * S[..., 3])
        pp = sum(c[i] * c[j] * S[..., i + j] for i in range(3) for j in range(3))
        return Sr, Srx, S[..., 8] - 2 * (c[0] * S[..., 5] + c[1] * S[..., 6] + c[2] * S[..., 7]) + pp

    Sr, Srx, Srr = remainder(S)
    n = S[:, 0]
    with np.errstate(all="ignore"):
        mx = S[:, 1] / n
        var = S[:, 2] / n - mx * mx
        enough = n >= max(min_count, 1)
        status = np.where(enough, np.where((var >= min_spread ** 2) & (var > 0), 0, 1), 2)
        b = np.where(status == 0, (Srx / n - mx * Sr / n) / var, 0.0)
        a = np.where(status < 2, Sr / n - b * mx, 0.0)
    a = np.nan_to_num(a); b = np.nan_to_num(b)
    rest = Srr - 2 * (a * Sr + b * Srx) + a * a * n + 2 * a * b * S[:, 1] + b * b * S[:, 2]
    _, _, Trr = remainder(T)
    rms = np.sqrt(np.maximum(np.array([T[8], Trr, rest.sum()]), 0.0) / T[0])
    return dict(c=c, a=a, b=b, status=status.astype(np.int32), rms=rms, degree=degree)


def cell_terms(setup, a, b, interp):
    """(A, B) [h, w] of every pixel"""
    w, h = setup.size
    bx, by = setup.bins
    a = np.asarray(a).reshape(by, bx); b = np.asarray(b).reshape(by, bx)
    if interp == CELL:
        cm = setup.cell_map()
        return a.ravel()[cm], b.ravel()[cm]
    fx = np.clip((np.arange(w) + 0.5) * bx / w - 0.5, 0, bx - 1); fy = np.clip((np.arange(h) + 0.5) * by / h - 0.5, 0, by - 1)
    k0 = np.floor(fx).astype(int); k1 = np.minimum(k0 + 1, bx - 1); l0 = np.floor(fy).astype(int); l1 = np.minimum(l0 + 1, by - 1)
    ax = (fx - k0)[None, :]; ay = (fy - l0)[:, None]

    def mix(t):
        return (1 - ay) * ((1 - ax) * t[l0][:, k0] + ax * t[l0][:, k1]) + ay * ((1 - ax) * t[l1][:, k0] + ax * t[l1][:, k1])
    return mix(a), mix(b)


def correct(setup, f, depth, interp):
    """depth [h, w] uint16 -> dict(out uint16, sum = v + delta before the rounding (NaN for v = 0), counters [3])"""
    v = np.asarray(depth).astype(np.float64)
    A, B = cell_terms(setup, f["a"], f["b"], interp)
    x = (v - setup.v_ref) / setup.v_ref
    c = f["c"]
    total = v + (c[0] + c[1] * x + c[2] * x * x + A + B * x)
    r = np.floor(total + 0.5)
    zero = v == 0
    bad = ~zero & ~((r >= 1) & (r <= 65535))
    out = np.where(zero | bad, 0, r).astype(np.uint16)
    return dict(out=out, sum=np.where(zero, np.nan, total), counters=np.array([zero.sum(), (~zero & ~bad).sum(), bad.sum()], dtype=np.int64))
