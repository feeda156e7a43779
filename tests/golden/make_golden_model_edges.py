"""Generate the reference for the camera models at their branch points (tests/golden/model_edges.json) with mpmath at 120 digits.

Independent of oracle/ and of the HIP code, like make_golden_math.py: the six projections are written out from the published Calibu
definitions with the branches vc_math.hpp documents (fov: w*w > 1e-5 and r^2 < 1e-5; kb4 on the axis gives the principal point), the
residual of a corner is a function of a pose increment (T <- T * exp([v, w]), the convention of se3_plus), of the camera's extrinsics
(R_ck <- R_ck exp(w), t_ck <- t_ck + t) and of the intrinsics, and every Jacobian is a central difference of that function in mpmath
(step 1e-25 of the operand's size) -- no closed form is restated.  The robust weights are SoftLOne(0.5) as corner_rows applies them:
w = rho'(|r|^2), H = sum w J^T J, g = sum w J^T r, cost = 1/2 sum rho, no second-order correction.  Sums are formed in mpmath and
rounded once.  Inputs are stored as exact doubles (hex), expected values with 25 digits.  Run in the authoring container:
    python tests/golden/make_golden_model_edges.py
writes tests/golden/model_edges.json (committed); the tests read the JSON only.

Left out on purpose (outside the contract of the arithmetic): Z = 0 for the radial models (fast_rcp(0)), and kb4 with X*X + Y*Y in the
denormal range (X = 1e-160, say): the sum of squares loses the direction there, in the host build as well (A wrong by 1e-5).
"""
import json
import os
import mpmath as mp

mp.mp.dps = 120
HERE = os.path.dirname(os.path.abspath(__file__))
MODEL_IDS = {"fov": 0, "poly2": 1, "poly3": 2, "kb4": 3, "linear": 4, "rational6": 5}
MODEL_NAMES = {v: k for k, v in MODEL_IDS.items()}
NK = {"fov": 5, "poly2": 6, "poly3": 7, "kb4": 8, "linear": 4, "rational6": 10}
SMALL = mp.mpf(1e-5)          # the double both fov thresholds compare with
STEP = mp.mpf(10) ** -25


def M(x):
    return mp.mpf(x)          # a double, exactly


def S(x):
    return mp.nstr(x, 25)


# ---------------------------------------------------------------------------------------------- projections
def project(model, p, k):
    X, Y, Z = p
    if model == "kb4":
        rho = mp.sqrt(X * X + Y * Y)
        if rho == 0:
            if not Z > 0:
                raise ValueError("kb4: the ray opposite to the axis has no direction")
            return [k[2], k[3]]
        th = mp.atan2(rho, Z)
        t2 = th * th
        R = th * (1 + t2 * (k[4] + t2 * (k[5] + t2 * (k[6] + t2 * k[7]))))
        return [k[0] * R * X / rho + k[2], k[1] * R * Y / rho + k[3]]
    x, y = X / Z, Y / Z
    r2 = x * x + y * y
    if model == "fov":
        w = k[4]
        if w * w > SMALL:
            m = 2 * mp.tan(w / 2)
            if r2 < SMALL:
                fac = m / w
            else:
                r = mp.sqrt(r2)
                fac = mp.atan(r * m) / (r * w)
        else:
            fac = mp.mpf(1)
    elif model == "poly2":
        fac = 1 + r2 * (k[4] + r2 * k[5])
    elif model == "poly3":
        fac = 1 + r2 * (k[4] + r2 * (k[5] + r2 * k[6]))
    elif model == "rational6":
        fac = (1 + r2 * (k[4] + r2 * (k[5] + r2 * k[6]))) / (1 + r2 * (k[7] + r2 * (k[8] + r2 * k[9])))
    else:
        fac = mp.mpf(1)
    return [fac * k[0] * x + k[2], fac * k[1] * y + k[3]]


def central(f, x0, scale):
    """columns of d f / d x at x0 by central differences; scale[i]: the size of operand i"""
    cols = []
    for i in range(len(x0)):
        h = STEP * scale[i]
        xp = list(x0); xm = list(x0)
        xp[i] = x0[i] + h; xm[i] = x0[i] - h
        fp, fm = f(xp), f(xm)
        cols.append([(a - b) / (2 * h) for a, b in zip(fp, fm)])
    return [[cols[j][i] for j in range(len(x0))] for i in range(len(cols[0]))]       # rows


def project_jacobians(model, p, k):
    size = max(abs(c) for c in p)
    A = central(lambda q: project(model, q, k), p, [size] * 3)
    B = central(lambda q: project(model, p, q), k, [max(abs(c), mp.mpf(1)) for c in k])
    return A, B


# ---------------------------------------------------------------------------------------------- poses
def quat_to_R(q):
    x, y, z, w = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]


def matmul(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def matvec(A, v):
    return [sum(A[i][k] * v[k] for k in range(3)) for i in range(3)]


def tmatvec(A, v):
    return [sum(A[k][i] * v[k] for k in range(3)) for i in range(3)]


def exp_and_V(w):
    """exp([w]x) and V = I + a [w]x + b [w]x^2, a = (1 - cos th) / th^2, b = (th - sin th) / th^3"""
    t = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    O = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    O2 = matmul(O, O)
    if t == 0:
        s, a, b = mp.mpf(1), mp.mpf(1) / 2, mp.mpf(1) / 6
    else:
        th = mp.sqrt(t)
        s, a, b = mp.sin(th) / th, (1 - mp.cos(th)) / t, (th - mp.sin(th)) / (t * th)
    E = [[(1 if i == j else 0) + s * O[i][j] + a * O2[i][j] for j in range(3)] for i in range(3)]
    V = [[(1 if i == j else 0) + a * O[i][j] + b * O2[i][j] for j in range(3)] for i in range(3)]
    return E, V


def residual(model, k, T_wk, T_ck, pw, uv, d):
    """r(d), d = [v_wk (3), w_wk (3), w_ck (3), t_ck (3), dK (nk)]: T_wk <- T_wk exp([v, w]), R_ck <- R_ck exp(w_ck), t_ck <- t_ck + t,
    K <- K + dK;  p_c = R_ck (R_wk^T (p_w - t_wk)) + t_ck,  r = Project(p_c, K) - z"""
    Rwk, twk = quat_to_R(T_wk[:4]), T_wk[4:]
    Rck, tck = quat_to_R(T_ck[:4]), T_ck[4:]
    if any(c != 0 for c in d[:6]):
        E, V = exp_and_V(d[3:6])
        dt = matvec(Rwk, matvec(V, d[0:3]))
        Rwk = matmul(Rwk, E); twk = [twk[i] + dt[i] for i in range(3)]
    if any(c != 0 for c in d[6:9]):
        Rck = matmul(Rck, exp_and_V(d[6:9])[0])
    tck = [tck[i] + d[9 + i] for i in range(3)]
    kk = [k[i] + d[12 + i] for i in range(len(k))]
    y = tmatvec(Rwk, [pw[i] - twk[i] for i in range(3)])
    q = matvec(Rck, y)
    pix = project(model, [q[i] + tck[i] for i in range(3)], kk)
    return [pix[0] - uv[0], pix[1] - uv[1]]


def corner(model, k, T_wk, T_ck, pw, uv):
    """(r, J (2 x (12 + nk)), rho, w) of one corner; J by central differences, SoftLOne(0.5) on s = |r|^2"""
    nk = len(k)
    size = max(max(abs(c) for c in pw), max(abs(c) for c in T_wk[4:]), max(abs(c) for c in T_ck[4:]))
    scale = [size] * 3 + [mp.mpf(1)] * 6 + [size] * 3 + [max(abs(c), mp.mpf(1)) for c in k]
    zero = [mp.mpf(0)] * (12 + nk)
    r = residual(model, k, T_wk, T_ck, pw, uv, zero)
    J = central(lambda d: residual(model, k, T_wk, T_ck, pw, uv, d), zero, scale)
    s = r[0] * r[0] + r[1] * r[1]
    t = mp.sqrt(1 + 4 * s)
    return r, J, (t - 1) / 2, 1 / t


def normal_equations(cams, poses, tiles):
    """cams: [(model name, K, T_ck)], poses: [T_wk], tiles: [(frame, camera, [p_w], [uv])], everything mpf.
    Returns per frame H (6 x 6) and g (6) over [v_wk, w_wk]; per camera H (n x n) and g (n) over [w_ck, t_ck, K]; the cost."""
    Hf = [[[mp.mpf(0)] * 6 for _ in range(6)] for _ in poses]
    gf = [[mp.mpf(0)] * 6 for _ in poses]
    Hc = [[[mp.mpf(0)] * (6 + len(c[1])) for _ in range(6 + len(c[1]))] for c in cams]
    gc = [[mp.mpf(0)] * (6 + len(c[1])) for c in cams]
    cost = mp.mpf(0)
    for (f, c, pws, uvs) in tiles:
        model, k, T_ck = cams[c]
        n = 6 + len(k)
        for pw, uv in zip(pws, uvs):
            r, J, rho, w = corner(model, k, poses[f], T_ck, pw, uv)
            cost += rho / 2
            for row in range(2):
                jf, jc = J[row][:6], J[row][6:]
                for i in range(6):
                    gf[f][i] += w * jf[i] * r[row]
                    for j in range(6):
                        Hf[f][i][j] += w * jf[i] * jf[j]
                for i in range(n):
                    gc[c][i] += w * jc[i] * r[row]
                    for j in range(n):
                        Hc[c][i][j] += w * jc[i] * jc[j]
    return Hf, gf, Hc, gc, cost


# ---------------------------------------------------------------------------------------------- the case table
IDENTITY = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
MID = [0.3, -0.2, 1.0]


def ring(r, cx, cy, z=1.0):
    return [r * cx, r * cy, z]


# every model: camera-frame points (rig and camera pose are the identity: p_c = p_w exactly)
POINTS = [
    ("axis_z1", [0.0, 0.0, 1.0]), ("axis_z2.5", [0.0, 0.0, 2.5]),
    ("r1e-9", ring(1e-9, 0.6, -0.8)), ("r1e-6", ring(1e-6, -0.8, 0.6)), ("r1e-4", ring(1e-4, 0.6, 0.8)), ("r3e-3", ring(3e-3, -0.6, -0.8)),
    # sqrt(1e-5) = 3.1623e-3: 1.3 % below and 1.2 % above, so that one ulp of x = X * rcp(Z) cannot change the branch
    ("r3.12e-3", ring(3.12e-3, 0.8, 0.6)), ("r3.2e-3", ring(3.2e-3, 0.8, -0.6)),
    ("mid", MID),
    # vc_atan's switch points (0.66, 2.414) seen through r * m: m = 0.99 for w = 0.92
    ("r0.66", ring(0.66, 0.8, 0.6)), ("r0.99", ring(0.99, -0.6, 0.8)), ("r2.7", ring(2.7, 0.6, -0.8)),
    ("r90", [5.0, -7.0, 0.1]),
    ("mid_2^40", [c * 2.0 ** 40 for c in MID]), ("mid_2^-40", [c * 2.0 ** -40 for c in MID]),
    # behind the camera: the radial models project it as it stands, for kb4 theta is in (pi/2, pi)
    ("z_neg", [0.3, -0.2, -0.5]),
    # vc_atan_ratio_pos's switch points rho / Z = 0.66 and 2.41421356 (kb4), either side
    ("rho0.65", ring(0.65, -0.6, -0.8)), ("rho0.67", ring(0.67, 0.6, 0.8)), ("rho2.40", ring(2.40, -0.8, -0.6)), ("rho2.43", ring(2.43, 0.8, -0.6)),
    ("rho1e-3_z-1", ring(1e-3, 0.6, -0.8, -1.0)),
]
KB4_ONLY = [("z0", [0.3, -0.2, 0.0])]

BASE = [330.0, 331.0, 320.5, 240.25]
CAMERAS = [
    ("fov_w0.92", "fov", BASE + [0.92]), ("fov_w2.6", "fov", BASE + [2.6]), ("fov_w-0.92", "fov", BASE + [-0.92]),
    # w*w <= 1e-5: fac = 1 and the w column is identically zero; 0.00317 is the first value of the table above the threshold
    ("fov_w0", "fov", BASE + [0.0]), ("fov_w0.003", "fov", BASE + [0.003]), ("fov_w0.00316", "fov", BASE + [0.00316]),
    ("fov_w0.00317", "fov", BASE + [0.00317]),
    ("poly2", "poly2", [400.0, 401.0, 320.5, 240.25, -0.28, 0.09]),
    ("poly3", "poly3", [400.0, 401.0, 320.5, 240.25, -0.28, 0.09, -0.012]),
    ("kb4", "kb4", [260.0, 261.0, 320.5, 240.25, -0.012, 0.004, -0.0015, 0.0002]),
    ("linear", "linear", [400.0, 401.0, 320.5, 240.25]),
    # the coefficients of the committed known answers (math_kat.json)
    ("rational6", "rational6", [400.0, 401.0, 320.5, 240.25, 0.12, 0.05, 0.004, 0.40, -0.04, 0.002]),
]

# the two frames of the Gram face, 8 corners at depth 1 each.  "axis": the corner on the axis, the small radii and both sides of the
# r^2 threshold, with three mid-field corners that determine the pose; "wide": mid field to r = 9 through vc_atan's switch points.
GRAM_FRAMES = [
    ("axis", [[0.0, 0.0, 1.0], ring(1e-9, 0.6, -0.8), ring(1e-6, -0.8, 0.6), ring(3.12e-3, 0.8, 0.6), ring(3.2e-3, 0.8, -0.6),
              MID, [-0.25, 0.3, 1.0], [0.2, 0.35, 1.0]]),
    ("wide", [MID, ring(0.66, 0.8, 0.6), ring(0.99, -0.6, 0.8), ring(2.7, 0.6, -0.8), ring(9.0, -0.6, -0.8), [-0.4, -0.5, 1.0],
              ring(1.5, -0.8, 0.6), ring(0.5, 0.0, -1.0)]),
]
# detections = the exact projection (rounded) + an offset in pixels: the whole range of the robust weight inside one frame
OFFSETS = [(0.0, 0.0), (6e-4, -8e-4), (0.6, 0.8), (-800.0, 600.0), (6e5, 8e5), (0.0, 0.0), (-8e-4, -6e-4), (-0.8, 0.6)]


def hexes(v):
    return [float(c).hex() for c in v]


def build_fixture():
    out = {"cameras": []}
    for name, model, k in CAMERAS:
        km = [M(c) for c in k]
        w_fixed = model == "fov" and k[4] * k[4] <= 1e-5
        cam = {"name": name, "model": MODEL_IDS[model], "k": hexes(k), "fix_k": w_fixed, "points": [], "frames": []}
        sq, cost = mp.mpf(0), mp.mpf(0)
        for tag, p in POINTS + (KB4_ONLY if model == "kb4" else []):
            pm = [M(c) for c in p]
            pix = project(model, pm, km)
            A, B = project_jacobians(model, pm, km)
            s = pix[0] * pix[0] + pix[1] * pix[1]
            sq += s; cost += (mp.sqrt(1 + 4 * s) - 1) / 4
            cam["points"].append({"tag": tag, "p": hexes(p), "pix": [S(v) for v in pix], "A": [S(v) for row in A for v in row],
                                  "B": [S(v) for row in B for v in row]})
        cam["pixel_sum_sq"] = S(sq); cam["pixel_cost"] = S(cost)
        poses = [[M(c) for c in IDENTITY] for _ in GRAM_FRAMES]
        tiles = []
        for f, (tag, pts) in enumerate(GRAM_FRAMES):
            uv = []
            for p, off in zip(pts, OFFSETS):
                pix = project(model, [M(c) for c in p], km)
                uv.append([float(pix[0]) + off[0], float(pix[1]) + off[1]])
            tiles.append((f, 0, [[M(c) for c in p] for p in pts], [[M(c) for c in z] for z in uv]))
            cam["frames"].append({"tag": tag, "pw": [hexes(p) for p in pts], "uv": [hexes(z) for z in uv]})
        total = mp.mpf(0)
        Hk = [[mp.mpf(0)] * len(k) for _ in k]; gk = [mp.mpf(0)] * len(k)
        for f, tile in enumerate(tiles):     # frame by frame: the per-frame cost is part of the fixture
            Hf, gf, Hc, gc, c = normal_equations([(model, km, [M(v) for v in IDENTITY])], poses, [tile])
            fr = cam["frames"][f]
            fr["Hpp"] = [S(v) for row in Hf[f] for v in row]; fr["gp"] = [S(v) for v in gf[f]]; fr["cost"] = S(c)
            # the whole block over [v, w | K] of this frame: what the host harness's tile Gram holds after its rotations
            fr["Hkk"] = [S(Hc[0][6 + i][6 + j]) for i in range(len(k)) for j in range(len(k))]
            fr["gk"] = [S(v) for v in gc[0][6:]]
            total += c
            for i in range(len(k)):
                gk[i] += gc[0][6 + i]
                for j in range(len(k)):
                    Hk[i][j] += Hc[0][6 + i][6 + j]
        cam["hss_diag"] = [S(Hk[i][i]) for i in range(len(k))]; cam["g_s"] = [S(v) for v in gk]; cam["cost"] = S(total)
        out["cameras"].append(cam)
    return out


def dumps(out):
    return json.dumps(out, indent=0) + "\n"


def main():
    out = build_fixture()
    with open(os.path.join(HERE, "model_edges.json"), "w") as f:
        f.write(dumps(out))
    print({c["name"]: (len(c["points"]), len(c["frames"])) for c in out["cameras"]})


if __name__ == "__main__":
    main()
