"""The camera models at their branch points: the committed mpmath reference (tests/golden/model_edges.json, written by
tests/golden/make_golden_model_edges.py) as arrays, and the deviation measures the host and the device tests share.

Deviations are measured against the fixture, on these scales:
  pixel        max(|pix|, 1)
  A, B         the block's largest entry
  H entries    sqrt(H_ii H_jj)
  g entries    sqrt(H_ii) * sqrt(2 * cost)
  cost         the cost
The bounds are the device bounds of the build's contract -- a few ulp for contraction, the Newton reciprocals and another tan on top of
what the host build shows (DESIGN.md section 5 has the measured maxima of both builds).  Every entry that involves fov's w column
carries (1 + 1 / w^2): m / w and dm / w cancel to w / 6 there (1.4e-11 of the column at w = 0.00317, host build).  No bound exceeds 1e-8,
what the linearisation is held to against the oracle on generic boards."""
import json
import os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
PIXEL_BOUND = 1e-14
# A and B (host only: no device face delivers them apart): a chain of ~30 operations of 1.1e-16 each; dpix/dZ = -(u_x x + u_y y) / Z
# multiplies the rounding of the block's largest entries by r, 86 in the table: 4 * 1.1e-16 * 86 = 3.8e-14
BLOCK_BOUND = 1e-13
H_BOUND = 1e-11
G_BOUND = 1e-11
COST_BOUND = 1e-12
CAP = 1e-8
_fixture = None


def _hex(v):
    return np.array([float.fromhex(c) for c in v])


def _num(v):
    return np.array([float(c) for c in v])


def cameras():
    """the fixture's cameras: name, model, k, fix_k, points (p [n, 3], pix [n, 2], A [n, 2, 3], B [n, 2, nk], tags), frames (pw [8, 3],
    uv [8, 2], Hpp [6, 6], gp [6], Hkk [nk, nk], gk [nk], cost), hss_diag, g_s, cost, pixel_sum_sq, pixel_cost"""
    global _fixture
    if _fixture is None:
        raw = json.load(open(os.path.join(HERE, "golden", "model_edges.json")))
        out = []
        for c in raw["cameras"]:
            k = _hex(c["k"]); nk = len(k)
            pts = c["points"]
            cam = dict(name=c["name"], model=c["model"], k=k, nk=nk, fix_k=c["fix_k"], tags=[p["tag"] for p in pts],
                       p=np.array([_hex(p["p"]) for p in pts]), pix=np.array([_num(p["pix"]) for p in pts]),
                       A=np.array([_num(p["A"]).reshape(2, 3) for p in pts]), B=np.array([_num(p["B"]).reshape(2, nk) for p in pts]),
                       hss_diag=_num(c["hss_diag"]), g_s=_num(c["g_s"]), cost=float(c["cost"]),
                       pixel_sum_sq=float(c["pixel_sum_sq"]), pixel_cost=float(c["pixel_cost"]), frames=[])
            for f in c["frames"]:
                cam["frames"].append(dict(tag=f["tag"], pw=np.array([_hex(p) for p in f["pw"]]), uv=np.array([_hex(p) for p in f["uv"]]),
                                          Hpp=_num(f["Hpp"]).reshape(6, 6), gp=_num(f["gp"]), Hkk=_num(f["Hkk"]).reshape(nk, nk),
                                          gk=_num(f["gk"]), cost=float(f["cost"])))
            out.append(cam)
        _fixture = out
    return _fixture


def camera_names():
    return [c["name"] for c in cameras()]


def camera(name):
    return next(c for c in cameras() if c["name"] == name)


def w_factor(cam):
    """(1 + 1 / w^2) of a fov camera with the w column alive, 1 otherwise; and the column's index among the intrinsics"""
    if cam["model"] == 0 and not cam["fix_k"]:
        return 1.0 + 1.0 / cam["k"][4] ** 2, 4
    return 1.0, -1


def _exact_where_zero(got, ref, what):
    z = ref == 0.0
    assert np.all(got[z] == 0.0), "%s: not exactly zero where the reference is: %r" % (what, got[z])


def dev_pixel(got, ref, k, what):
    """largest deviation of pixels [n, 2] on max(|pix|, 1) per corner; exact where the reference is the principal point or zero"""
    got = np.asarray(got, dtype=np.float64)
    assert np.all(np.isfinite(got)), "%s: non-finite pixel %r" % (what, got[~np.isfinite(got).all(axis=1)])
    pp = ref == k[2:4][None, :]
    assert np.all(got[pp] == ref[pp]), "%s: not exactly the principal point on the axis: %r" % (what, got[pp] - ref[pp])
    _exact_where_zero(got, ref, what)
    scale = np.maximum(np.abs(ref).max(axis=1), 1.0)[:, None]
    return np.abs(got - ref) / scale


def dev_block(got, ref, what):
    """deviation of a Jacobian block on its largest entry"""
    assert np.all(np.isfinite(got)), "%s: non-finite %r" % (what, got)
    _exact_where_zero(got, ref, what)
    return np.abs(got - ref) / np.abs(ref).max()


def dev_H(got, ref, what):
    """deviation of the entries of a Gram block on sqrt(H_ii H_jj); a vector is taken as a diagonal"""
    got = np.asarray(got, dtype=np.float64)
    assert np.all(np.isfinite(got)), "%s: non-finite %r" % (what, got)
    _exact_where_zero(got, ref, what)
    if ref.ndim == 1:
        scale = ref.copy()
    else:
        dg = np.sqrt(np.diag(ref)); scale = dg[:, None] * dg[None, :]
    return np.abs(got - ref) / np.where(scale > 0.0, scale, 1.0)


def dev_g(got, ref, h_diag, cost, what):
    """deviation of a gradient on sqrt(H_ii) sqrt(2 cost)"""
    got = np.asarray(got, dtype=np.float64)
    assert np.all(np.isfinite(got)), "%s: non-finite %r" % (what, got)
    _exact_where_zero(got, ref, what)
    scale = np.sqrt(h_diag) * np.sqrt(2.0 * cost)
    return np.abs(got - ref) / np.where(scale > 0.0, scale, 1.0)


def dev_cost(got, ref, what):
    assert np.isfinite(got), "%s: non-finite %r" % (what, got)
    return abs(got - ref) / ref


def k_bounds(cam, base, ndim):
    """bounds of a vector (ndim 1) or a matrix (ndim 2) over the intrinsics: base, times (1 + 1 / w^2) where fov's w column enters,
    capped at what the generic boards are held to"""
    fac, col = w_factor(cam)
    b = np.full(cam["nk"], base)
    if col >= 0:
        b[col] = min(base * fac, CAP)
    return b if ndim == 1 else np.maximum(b[:, None], b[None, :])


class Maxima:
    """the largest deviation per quantity, with the case that has it"""

    def __init__(self):
        self.m = {}

    def add(self, quantity, dev, bound, what):
        """records max(dev) (as it is and in units of its bound) and returns True when every entry is within its bound"""
        dev = np.atleast_1d(np.asarray(dev, dtype=np.float64)); bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), dev.shape)
        if dev.size == 0:
            return True
        i = int(np.argmax(dev / bound))
        rel = float((dev / bound).flat[i])
        if quantity not in self.m or rel > self.m[quantity][1]:
            self.m[quantity] = (float(dev.flat[i]), rel, what)
        return rel <= 1.0

    def lines(self):
        return ["%-22s %.3g (%.3g of its bound) at %s" % (q, v[0], v[1], v[2]) for q, v in sorted(self.m.items())]
