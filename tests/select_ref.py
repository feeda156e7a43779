"""An independent numpy statement of greedy D-optimal view selection (include/vicalib_amd.h: vc_selector*), for the tests of the host build and of
the kernels.  Two ways to the Jacobians: central differences of vicalib_amd.synth's projection with respect to a pose increment T <- T exp(d), the
extrinsics (R_ck <- R_ck exp(w), t_ck <- t_ck + dt) and K -- no closed form --, and an analytic variant that runs in float64 and in numpy.longdouble
(its own distance between the two is what the code under test is allowed, times 16).  Then the dense Schur complement, the scaling and the greedy
loop; log-determinants by numpy.linalg.slogdet in float64 and by a Cholesky written out here in long double."""
import numpy as np

from vicalib_amd import synth

ROT, TRANS, KFREE = 1, 2, 4
NK = synth.MODEL_NK
PIVOT_TOL = 1e-12


def model_id(m):
    return synth.MODEL_IDS[m] if isinstance(m, str) else int(m)


def ncols(model, flags):
    return (3 if flags & ROT else 0) + (3 if flags & TRANS else 0) + (NK[model_id(model)] if flags & KFREE else 0)


def dim(cameras):
    return sum(ncols(c[0], c[3]) for c in cameras)


def quat_R(q, dt):
    x, y, z, w = [dt(v) for v in q[:4]]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=dt)


def views_of(case):
    """{frame: [(camera, point ids in order of arrival)] ordered by camera}"""
    per = {}
    for f, c, ids in case["tiles"]:
        per.setdefault(f, {}).setdefault(c, []).extend(int(i) for i in ids)
    return {f: sorted(v.items()) for f, v in per.items()}


# ---------------------------------------------------------------------------------------------- Jacobians by central differences
def _pc(Rwk, twk, Rck, tck, pw):
    return (pw - twk) @ Rwk @ Rck.T + tck


def numeric_rows(case, f, c, ids, h):
    """(J_f [2n, 6], J_c [2n, ncols of camera c], in front [n]) of one view by central differences of step h (times max(1, |K_k|) for K)"""
    m, K, T_ck, flags = case["cameras"][c]
    m = model_id(m)
    K = np.asarray(K, dtype=np.float64)
    T = np.asarray(case["poses"][f], dtype=np.float64)
    Rwk, twk = quat_R(T, np.float64), T[4:7]
    Rck, tck = quat_R(T_ck, np.float64), np.asarray(T_ck[4:7], dtype=np.float64)
    pw = np.asarray(case["points"], dtype=np.float64)[ids]
    front = np.ones(len(ids), dtype=bool) if m == 3 else _pc(Rwk, twk, Rck, tck, pw)[:, 2] > 0.0

    def pix(dv=None, dw=None, dwc=None, dtc=None, dK=None):
        R1 = Rwk @ synth.so3_exp_matrix(dw) if dw is not None else Rwk
        t1 = twk + Rwk @ dv if dv is not None else twk
        Rc = Rck @ synth.so3_exp_matrix(dwc) if dwc is not None else Rck
        tc = tck + dtc if dtc is not None else tck
        with np.errstate(all="ignore"):
            return synth.project(m, K + dK if dK is not None else K, _pc(R1, t1, Rc, tc, pw)).reshape(-1)

    def col(key, k, n, step):
        e = np.zeros(n); e[k] = step
        return (pix(**{key: e}) - pix(**{key: -e})) / (2.0 * step)

    Jf = np.stack([col("dv", k, 3, h) for k in range(3)] + [col("dw", k, 3, h) for k in range(3)], axis=1)
    cols = []
    if flags & ROT:
        cols += [col("dwc", k, 3, h) for k in range(3)]
    if flags & TRANS:
        cols += [col("dtc", k, 3, h) for k in range(3)]
    if flags & KFREE:
        cols += [col("dK", k, len(K), h * max(1.0, abs(K[k]))) for k in range(len(K))]
    Jc = np.stack(cols, axis=1) if cols else np.zeros((2 * len(ids), 0))
    keep = np.repeat(front, 2)
    return Jf[keep], Jc[keep], front


# ---------------------------------------------------------------------------------------------- analytic Jacobians, any float type
def _proj_jac(m, K, P, dt):
    """A [n, 2, 3] = d pix / d p_c and B [n, 2, nk] = d pix / d K"""
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    n, nk = len(P), len(K)
    A, B = np.zeros((n, 2, 3), dtype=dt), np.zeros((n, 2, nk), dtype=dt)
    fu, fv = K[0], K[1]
    one = dt(1)
    if m == 3:
        rho2 = X * X + Y * Y
        rho = np.sqrt(rho2)
        n2 = rho2 + Z * Z
        th = np.arctan2(rho, Z)
        t2 = th * th
        poly = one + t2 * (K[4] + t2 * (K[5] + t2 * (K[6] + t2 * K[7])))
        R = th * poly
        dR = one + t2 * (3 * K[4] + t2 * (5 * K[5] + t2 * (7 * K[6] + t2 * 9 * K[7])))
        c, s = X / rho, Y / rho
        th_d = np.stack([Z * c / n2, Z * s / n2, -rho / n2], axis=1)
        c_d = np.stack([s * s / rho, -c * s / rho, np.zeros_like(X)], axis=1)
        s_d = np.stack([-c * s / rho, c * c / rho, np.zeros_like(X)], axis=1)
        A[:, 0, :] = fu * ((dR * c)[:, None] * th_d + R[:, None] * c_d)
        A[:, 1, :] = fv * ((dR * s)[:, None] * th_d + R[:, None] * s_d)
        B[:, 0, 0] = R * c; B[:, 0, 2] = one
        B[:, 1, 1] = R * s; B[:, 1, 3] = one
        for i in range(4):
            p = th ** (3 + 2 * i)
            B[:, 0, 4 + i] = fu * c * p; B[:, 1, 4 + i] = fv * s * p
        return A, B
    x, y = X / Z, Y / Z
    r2 = x * x + y * y
    dk = []                                                     # d fac / d K[4 + i]
    if m == 0:
        w = K[4]
        mm = 2 * np.tan(w / 2)
        dm = one + mm * mm / 4
        small = r2 < 1e-5
        r = np.sqrt(np.where(small, one, r2))
        at = np.arctan(r * mm)
        den = one + r2 * mm * mm
        fac = np.where(small, mm / w, at / (r * w))
        g = np.where(small, 0 * r2, (mm * r / (one + r * r * mm * mm) - at) / (r * r * r * w) / 2)      # d fac / d r2
        dk = [np.where(small, dm / w - mm / (w * w), dm / (den * w) - at / (r * w * w))]
    elif m in (1, 2):
        k3 = K[6] if m == 2 else dt(0)
        fac = one + r2 * (K[4] + r2 * (K[5] + r2 * k3))
        g = K[4] + r2 * (2 * K[5] + 3 * k3 * r2)
        dk = [r2, r2 * r2] + ([r2 * r2 * r2] if m == 2 else [])
    elif m == 5:
        N = one + r2 * (K[4] + r2 * (K[5] + r2 * K[6])); Dn = one + r2 * (K[7] + r2 * (K[8] + r2 * K[9]))
        dN = K[4] + r2 * (2 * K[5] + 3 * K[6] * r2); dD = K[7] + r2 * (2 * K[8] + 3 * K[9] * r2)
        fac = N / Dn
        g = (dN * Dn - N * dD) / (Dn * Dn)
        dk = [r2 / Dn, r2 * r2 / Dn, r2 * r2 * r2 / Dn, -N * r2 / (Dn * Dn), -N * r2 * r2 / (Dn * Dn), -N * r2 * r2 * r2 / (Dn * Dn)]
    else:
        fac = np.ones_like(r2); g = np.zeros_like(r2)
    # u = fu x fac + cu: du/dx = fu (fac + 2 g x^2), du/dy = fu 2 g x y; dx/dX = 1/Z, dx/dZ = -x/Z
    ux, uy = fu * (fac + 2 * g * x * x), fu * 2 * g * x * y
    vx, vy = fv * 2 * g * x * y, fv * (fac + 2 * g * y * y)
    A[:, 0, 0] = ux / Z; A[:, 0, 1] = uy / Z; A[:, 0, 2] = -(ux * x + uy * y) / Z
    A[:, 1, 0] = vx / Z; A[:, 1, 1] = vy / Z; A[:, 1, 2] = -(vx * x + vy * y) / Z
    B[:, 0, 0] = x * fac; B[:, 0, 2] = one
    B[:, 1, 1] = y * fac; B[:, 1, 3] = one
    for i, d in enumerate(dk):
        B[:, 0, 4 + i] = fu * x * d; B[:, 1, 4 + i] = fv * y * d
    return A, B


def analytic_rows(case, f, c, ids, dt):
    m, K, T_ck, flags = case["cameras"][c]
    m = model_id(m)
    K = np.array([dt(k) for k in K], dtype=dt)
    T = case["poses"][f]
    Rwk, twk = quat_R(T, dt), np.array([dt(v) for v in T[4:7]], dtype=dt)
    Rck, tck = quat_R(T_ck, dt), np.array([dt(v) for v in T_ck[4:7]], dtype=dt)
    pw = np.asarray(case["points"])[ids].astype(dt)
    q = (pw - twk) @ Rwk @ Rck.T
    pc = q + tck
    front = np.ones(len(ids), dtype=bool) if m == 3 else pc[:, 2] > 0
    pc, q = pc[front], q[front]
    A, B = _proj_jac(m, K, pc, dt)
    V = np.cross(A, q[:, None, :])                              # rows a_i x q
    Jf = np.concatenate([-(A @ Rck), V @ Rck], axis=2).reshape(-1, 6)
    cols = []
    if flags & ROT:
        cols.append(-(V @ Rck))
    if flags & TRANS:
        cols.append(A)
    if flags & KFREE:
        cols.append(B)
    Jc = np.concatenate(cols, axis=2).reshape(len(pc) * 2, -1) if cols else np.zeros((2 * len(pc), 0), dtype=dt)
    return Jf, Jc, front


# ---------------------------------------------------------------------------------------------- frame information
def _solve_spd(M, rhs, dt):
    """M^-1 rhs by a Cholesky written out (numpy.linalg has no long double); None when a pivot fails the status rule"""
    n = len(M)
    L = np.zeros((n, n), dtype=dt)
    floor = dt(PIVOT_TOL) * max(M[j, j] for j in range(n))
    for j in range(n):
        d = M[j, j] - L[j, :j] @ L[j, :j]
        if not d > floor:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (M[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros_like(rhs)
    for i in range(n):
        y[i] = (rhs[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros_like(rhs)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def frame_information(case, rows, dt=np.float64):
    """rows(case, f, c, ids) -> (Jf, Jc, front).  -> I [N, D, D], status [N], corners [N], behind [N]"""
    cams = case["cameras"]
    N, D = len(case["poses"]), dim(cams)
    col0 = np.cumsum([0] + [ncols(c[0], c[3]) for c in cams])
    I = np.zeros((N, D, D), dtype=dt)
    status, corners, behind = np.zeros(N, dtype=int), np.zeros(N, dtype=int), np.zeros(N, dtype=int)
    views = views_of(case)
    for f in range(N):
        Jfs, Jss = [], []
        for c, ids in views.get(f, []):
            Jf, Jc, front = rows(case, f, c, np.asarray(ids, dtype=int))
            corners[f] += int(front.sum()); behind[f] += int((~front).sum())
            Js = np.zeros((len(Jf), D), dtype=dt)
            Js[:, col0[c]:col0[c + 1]] = Jc
            Jfs.append(Jf.astype(dt)); Jss.append(Js)
        ok = corners[f] >= 4
        if ok:
            Jf, Js = np.concatenate(Jfs), np.concatenate(Jss)
            W = Jf.T @ Js
            X = _solve_spd(Jf.T @ Jf, W, dt)
            ok = X is not None
            if ok:
                I[f] = Js.T @ Js - W.T @ X
        status[f] = 1 if not ok else (2 if behind[f] > 0 else 0)
    return I, status, corners, behind


def scaling(I, status):
    d = np.einsum("fjj->j", I[status != 1]) if (status != 1).any() else np.zeros(I.shape[1], dtype=I.dtype)
    one = I.dtype.type(1)
    return np.where(d > 0, one / np.sqrt(np.where(d > 0, d, one)), one)


def scaled(I, s):
    return I * s[None, :, None] * s[None, None, :]


# ---------------------------------------------------------------------------------------------- log-determinants and the greedy loop
def logdet(M):
    """log det of symmetric positive definite matrices [..., D, D]: slogdet in float64, a Cholesky written out otherwise"""
    if M.dtype == np.float64:
        return np.linalg.slogdet(M)[1]
    M = M.copy()
    D = M.shape[-1]
    out = np.zeros(M.shape[:-2], dtype=M.dtype)
    for k in range(D):
        p = M[..., k, k].copy()
        out += np.log(p)
        r = M[..., k, k + 1:].copy()
        M[..., k + 1:, k + 1:] -= r[..., :, None] * r[..., None, :] / p[..., None, None]
    return out


def start_matrix(It, start, prior):
    D = It.shape[1]
    S = np.eye(D, dtype=It.dtype) * It.dtype.type(prior)
    for f in start:
        S = S + It[f]
    return S


def gains_given(It, status, S, chosen):
    """the gain of every frame against S; -1 for frames in `chosen` or unusable"""
    N = len(It)
    cand = np.array([f for f in range(N) if f not in chosen and status[f] != 1], dtype=int)
    g = np.full(N, -1.0, dtype=It.dtype)
    if len(cand):
        g[cand] = logdet(S[None] + It[cand]) - logdet(S)
    return g


def total_of(It, status, start, prior):
    S0 = start_matrix(It, start, prior)
    rest = [f for f in range(len(It)) if f not in set(start) and status[f] != 1]
    return logdet(S0 + sum((It[f] for f in rest), np.zeros_like(S0))) - logdet(S0)


def greedy(It, status, k, start=(), prior=1e-6, sequence=None):
    """-> dict(order, gain, cum, total, rounds=[gains of every frame per round]).  sequence: follow these picks instead of the argmax"""
    S0 = start_matrix(It, start, prior)
    S, chosen = S0, set(int(f) for f in start)
    order, gain, cum, rounds = [], [], [], []
    for r in range(min(k, len(It))):
        g = gains_given(It, status, S, chosen)
        if not (g >= 0).any():
            break
        f = int(np.argmax(g)) if sequence is None else int(sequence[r]) if r < len(sequence) else -1
        rounds.append(g)
        if f < 0 or not g[f] > 0:
            break
        S = S + It[f]
        chosen.add(f)
        order.append(f); gain.append(g[f]); cum.append(logdet(S) - logdet(S0))
    return dict(order=np.array(order, dtype=int), gain=np.array(gain, dtype=It.dtype), cum=np.array(cum, dtype=It.dtype),
                total=total_of(It, status, start, prior), rounds=rounds)
