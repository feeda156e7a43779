"""TEST INFRASTRUCTURE shared by test_uncertainty_cpu.py and test_uncertainty_gpu.py: the cameras and covariances of the projection-uncertainty
map, the numpy side of every check (the oracle's projection with its Jacobians over the rays of compare_cases._inverted, the oracle's inversion
by bisection) and the checks themselves -- written against plain arrays, so that the same check holds the host build of the map's arithmetic
(tests/host_harness/uncertainty_harness.cpp) and the GPU kernels.

A run is handed to the checks as a dict: M [3, nk], G [3, 3], n_fit; sigma [n, 3] and flags [n] in sample order; summary (count, invalid,
sum_var, max_lam, worst); rings {n_rings: dict(count, invalid, sum_var, max_lam)}."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import compare_cases as cc       # noqa: E402
import oracle_lib as ol          # noqa: E402
import undistort_cases as uc     # noqa: E402
from vicalib_amd import synth    # noqa: E402

SIZE = cc.SIZE
GRID = cc.GRID                                    # 53 x 41 = 2173 samples: a partial wave, a partial workgroup
ONE_WORKGROUP = (64, 16)                          # exactly 1024 samples
TINY = (2, 2)
NK = {"fov": 5, "poly2": 6, "poly3": 7, "kb4": 8, "linear": 4, "rational6": 10}
FIT_RADII = (1.0, 0.5, 0.0)                       # 0: no compensation
RING_COUNTS = cc.RING_COUNTS
FLAG_A, FLAG_INVALID = cc.FLAG_A, cc.FLAG_INVALID

# Check 1's tolerance.  MEASURED: the largest relative deviation of the host harness from the numpy reference over every case below (the two
# share only the model definitions; their rays agree to the inversion's round trip of 1e-8 px) -- of M per column against the column's largest
# entry, of G against its largest entry, of a triple against the sample's var = s_uu + s_vv.  Printed by test_uncertainty_cpu.py
# (test_host_arithmetic, -s).  The bound is fifty times that (the convention of convert_cases.POLY3_RATIONAL6_MEASURED) and holds the device too.
MEASURED = 5.4e-13                                # rational6 at fit radius 0.5; every other case 7e-14 to 2.5e-13 with compensation
TOLERANCE = 50.0 * MEASURED

# One dense covariance per model, Cov = (D L)(D L)^T: L lower triangular from numpy.random.default_rng(20261018) -- the models in the order
# below, row r: r draws of uniform(-1, 1), then the diagonal entry from uniform(0.5, 1), two decimals --, D the plausible size of each parameter: 0.3 px for fu and fv, 0.5 px for u0 and v0, 1e-3 for a
# distortion term.
_L = {
    "fov": [[0.94],
            [-0.23, 0.52],
            [0.47, 0.72, 0.88],
            [0.33, -0.96, -1, 0.98],
            [0.74, 0.45, -0.69, -0.51, 0.56]],
    "poly2": [[0.89],
              [0.53, 0.59],
              [-0.95, 0.64, 0.57],
              [-0.86, -0.76, -0.71, 0.7],
              [0.7, -0.03, 0.68, -0.5, 0.51],
              [0.41, -0.89, -0.02, 0.1, 0.23, 0.83]],
    "poly3": [[0.8],
              [0.73, 0.76],
              [0.52, -0.78, 0.53],
              [0.84, -0.29, 0.28, 0.52],
              [-0.33, 0.41, 0.48, 0.68, 0.75],
              [0.58, -0.06, 0.98, 0.12, 0.7, 0.77],
              [0.6, -0.88, 0.12, -0.51, 0.76, 0.54, 0.87]],
    "kb4": [[0.5],
            [0.92, 0.89],
            [0.14, 0.43, 0.57],
            [-0.57, 0.26, -0.26, 0.55],
            [-0.79, 0.68, -0.03, 0.48, 0.96],
            [-0.48, 0.95, 0.09, 0.58, -0.74, 0.72],
            [0.99, 0.58, 0.61, 0.99, -0.21, 0.41, 0.85],
            [-0.01, 0.62, -0.11, 0.97, -0.66, 0.81, -0.44, 0.87]],
    "linear": [[0.62],
               [0.99, 0.87],
               [0.51, 0.24, 0.66],
               [-0.89, 0.78, 0.87, 0.57]],
    "rational6": [[0.53],
                  [-0.4, 0.77],
                  [1, -0.04, 0.91],
                  [0.78, 0.67, -0.14, 0.56],
                  [0.95, -0.23, -0.16, 0.45, 0.89],
                  [-0.92, -0.69, -0.31, 0.77, 0.59, 0.65],
                  [0.83, -0.52, -0.53, 0.61, -0.68, -0.61, 0.97],
                  [0.09, -0.94, -0.1, -0.02, 0.49, 0.38, 0.87, 0.58],
                  [0.99, 0.38, 0.59, -0.09, 0.4, 0.49, 0.71, -0.96, 0.54],
                  [-0.48, 0.49, -0.25, 0.98, 0.18, -0.96, 0.41, 0.38, 0.87, 0.68]],
}


@functools.lru_cache(maxsize=None)
def dense_cov(model):
    nk = NK[model]
    L = np.zeros((nk, nk))
    for r, row in enumerate(_L[model]):
        L[r, : r + 1] = row
    D = np.array([0.3, 0.3, 0.5, 0.5] + [1e-3] * (nk - 4))
    DL = D[:, None] * L
    return DL @ DL.T


class Case:
    def __init__(self, name, model, K, fit_radius, grid=GRID, beyond=False):
        self.name, self.model, self.K, self.fit_radius, self.grid, self.beyond = name, model, np.asarray(K, dtype=np.float64), fit_radius, grid, beyond
        self.cov = dense_cov(model)
        self.sigma_px = 1.0

    @property
    def camera(self):
        return (self.model, self.K)


def case_names():
    return ["%s-%g" % (m, r) for m in uc.MODELS for r in FIT_RADII] + ["beyond", "one-workgroup", "tiny"]


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "beyond":
        return Case(name, "poly3", uc.BEYOND_K.copy(), 0.4, beyond=True)
    if name == "one-workgroup":
        return Case(name, "poly3", uc.gt("poly3"), 1.0, grid=ONE_WORKGROUP)
    if name == "tiny":
        return Case(name, "poly3", uc.gt("poly3"), 1.0, grid=TINY)
    m, r = name.rsplit("-", 1)
    return Case(name, m, uc.gt(m), float(r))


# ------------------------------------------------------------------------------------------------------------ numpy reference
def jacobians(model, K, rays):
    """the oracle's projection of every ray with its Jacobians: pix [n, 2], dray [n, 2, 3], dk [n, 2, nk] (vco_project, row-major blocks)"""
    import ctypes as C
    L = ol.lib()
    m = synth.MODEL_IDS[model]
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 3)
    K = np.ascontiguousarray(K, dtype=np.float64)
    n, nk = len(rays), L.vco_model_num_params(m)
    pix, dray, dk = np.zeros((n, 2)), np.zeros((n, 2, 3)), np.zeros((n, 2, nk))
    pK, fn = C.c_void_p(K.ctypes.data), L.vco_project
    r0, p0, a0, b0 = rays.ctypes.data, pix.ctypes.data, dray.ctypes.data, dk.ctypes.data
    for i in range(n):
        fn(m, C.c_void_p(r0 + 24 * i), pK, C.c_void_p(p0 + 16 * i), C.c_void_p(a0 + 48 * i), C.c_void_p(b0 + 16 * nk * i))
    return pix, dray, dk


def cross_matrix(a):
    """[a]x of every ray [n, 3] -> [n, 3, 3]"""
    z = np.zeros(len(a))
    return np.stack([np.stack([z, -a[:, 2], a[:, 1]], 1), np.stack([a[:, 2], z, -a[:, 0]], 1), np.stack([-a[:, 1], a[:, 0], z], 1)], 1)


@functools.lru_cache(maxsize=None)
def _rows(model, K, grid):
    """what does not depend on the fit radius: q, rho, rays, ok (the inversion), valid, B [n, 2, nk], Jw [n, 2, 3]"""
    q, rho = cc.lattice(SIZE, grid)
    rays, ok = cc._inverted(model, K, SIZE, grid)
    valid = ok & ((rays[:, 2] > 0) | (model == "kb4"))
    _, A, B = jacobians(model, np.array(K), rays)
    Jw = -np.einsum("nij,njk->nik", A, cross_matrix(rays))
    return q, rho, rays, ok, valid, B, Jw


class Reference:
    """of one camera on one lattice at one fit radius: q, rho, rays, ok, valid, undecided, fit (the fit set), G, C, M, J [n, 2, nk]"""

    def __init__(self, model, K, grid, fit_radius, beyond=False):
        self.model, self.K, self.grid, self.fit_radius = model, np.asarray(K, dtype=np.float64), grid, fit_radius
        self.q, self.rho, self.rays, self.ok, self.valid, self.B, self.Jw = _rows(model, tuple(K), grid)
        r = np.hypot(*(self.q - self.K[2:4]).T)
        self.undecided = np.zeros(len(self.q), dtype=bool)
        if beyond:
            self.undecided = (r > 0.9 * cc.R_MAX) & (r < 1.01 * cc.R_MAX)
            cc.assert_increasing(model, self.K, 0.9 * cc.R_MAX)
            assert self.undecided.mean() <= 0.10, self.undecided.mean()
        else:
            cc.assert_increasing(model, self.K, r.max())
            assert self.ok.all()
        assert max(self.K[0], self.K[1]) < 500                   # (the round trip of 1e-8 px assumes it)
        nk = NK[model]
        if fit_radius > 0:
            if grid == GRID:
                cc.assert_thresholds_decided(self.rho, fit_radius)
            self.fit = self.valid & (self.rho <= fit_radius)
            assert not (self.fit & self.undecided).any() and not ((self.rho <= fit_radius) & self.undecided).any()      # the fit set holds no undecided sample
            self.G = np.einsum("nri,nrj->ij", self.Jw[self.fit], self.Jw[self.fit])
            self.C = np.einsum("nri,nrk->ik", self.Jw[self.fit], self.B[self.fit])
            self.M = -np.linalg.solve(self.G, self.C)
        else:
            self.fit = np.zeros(len(self.q), dtype=bool)
            self.G, self.C, self.M = np.zeros((3, 3)), np.zeros((3, nk)), np.zeros((3, nk))
        self.J = self.B + np.einsum("nri,ik->nrk", self.Jw, self.M)

    def triples(self, cov, sigma_px=1.0):
        """[n, 3] = (s_uu, s_uv, s_vv), NaN where not valid"""
        S = sigma_px ** 2 * np.einsum("nrk,kl,nsl->nrs", self.J, np.asarray(cov), self.J)
        t = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 1, 1]], 1)
        t[~self.valid] = np.nan
        return t


def var_lam(t):
    t = np.asarray(t)
    var = t[:, 0] + t[:, 2]
    return var, np.maximum(0.5 * (var + np.sqrt((t[:, 0] - t[:, 2]) ** 2 + 4.0 * t[:, 1] ** 2)), 0.0)


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    return Reference(c.model, c.K, c.grid, c.fit_radius, c.beyond)


# ------------------------------------------------------------------------------------------------------------ checks
def deviation(ref, cov, sigma_px, out):
    """Check 1 without its bound: n_fit and the flags exactly (flags on decided samples), then the largest relative deviation of M (per column,
    against the column's largest entry), G (against its largest entry) and every triple valid on both sides (against the sample's var)"""
    flags, sg = np.asarray(out["flags"]).ravel(), np.asarray(out["sigma"]).reshape(-1, 3)
    dec = ~ref.undecided
    assert out["n_fit"] == ref.fit.sum()
    assert np.array_equal(((flags & FLAG_A) != 0)[dec], ~ref.ok[dec])
    bad = (flags & FLAG_INVALID) != 0
    assert np.array_equal(bad[dec], ~ref.valid[dec]) and np.all(bad[(flags & FLAG_A) != 0]) and not (flags.astype(int) & ~(FLAG_A | FLAG_INVALID)).any()
    assert np.isnan(sg[bad]).all() and np.isfinite(sg[~bad]).all()
    dev = 0.0
    if ref.fit_radius > 0:
        dev = max(dev, (np.abs(out["M"] - ref.M).max(axis=0) / np.abs(ref.M).max(axis=0)).max(), np.abs(out["G"] - ref.G).max() / np.abs(ref.G).max())
    else:
        assert not np.any(out["M"]) and not np.any(out["G"])
    t = ref.triples(cov, sigma_px)
    both = dec & ~bad & ref.valid
    var = t[both, 0] + t[both, 2]
    if np.any(var > 0):
        dev = max(dev, (np.abs(sg[both] - t[both]).max(axis=1) / var).max())
    else:
        assert not np.any(sg[both])
    return float(dev)


def check_map(ref, cov, sigma_px, out, name=""):
    """1. M, G, n_fit and every valid sample's triple against numpy; flags equal on decided samples"""
    dev = deviation(ref, cov, sigma_px, out)
    print("%s: largest relative deviation from numpy %.3g (bound %.3g)" % (name, dev, TOLERANCE))
    assert dev <= TOLERANCE
    return dev


def check_sums(ref, cov, sigma_px, out, dense=True):
    """2. summary and rings against numpy sums over the reference's own triples (at an undecided sample that the run calls valid, where the
    reference has none to offer: the run's own), with check 1's tolerance; the worst sample must match when the reference's top two lam differ
    by more than the tolerance -- asserted for the dense covariances -- and otherwise be one of the tied ones"""
    flags, sg = np.asarray(out["flags"]).ravel(), np.asarray(out["sigma"]).reshape(-1, 3)
    t = ref.triples(cov, sigma_px)
    ok = np.where(ref.undecided, (flags & FLAG_INVALID) == 0, ref.valid)
    t[ref.undecided & ok] = sg[ref.undecided & ok]
    var, lam = var_lam(t)
    s = out["summary"]
    assert s["count"] == ok.sum() and s["invalid"] == (~ok).sum()
    if not ok.any():
        assert s["worst"] == -1 and s["max_lam"] == 0 and s["sum_var"] == 0
        return
    assert abs(s["sum_var"] - var[ok].sum()) <= TOLERANCE * var[ok].sum()
    top = np.sort(lam[ok])[-2:]
    assert abs(s["max_lam"] - top[-1]) <= TOLERANCE * top[-1]
    decided = len(top) < 2 or top[1] - top[0] > TOLERANCE * top[1]
    if dense:
        assert decided, (top, TOLERANCE)                         # CPU precondition of the dense covariances: their worst sample is decided
    if decided:
        assert s["worst"] == np.nonzero(ok)[0][np.argmax(lam[ok])]
    else:
        assert ok[s["worst"]] and lam[s["worst"]] >= top[1] * (1.0 - TOLERANCE)
    for n, r in out["rings"].items():
        k = cc.ring_of(ref.rho, n)
        assert r["count"].sum() == s["count"] and r["invalid"].sum() == s["invalid"]
        for ring in range(n):
            m = ok & (k == ring)
            assert r["count"][ring] == m.sum() and r["invalid"][ring] == (~ok & (k == ring)).sum(), (n, ring)
            assert abs(r["sum_var"][ring] - var[m].sum()) <= TOLERANCE * var[m].sum(), (n, ring)
            want = lam[m].max() if m.any() else 0.0
            assert abs(r["max_lam"][ring] - want) <= TOLERANCE * want, (n, ring)


def check_case(name, run):
    """Checks 1 and 2 of one case.  run(case, cov, sigma_px, fit_radius) -> the dict above, rings at RING_COUNTS."""
    c, ref = case(name), reference(name)
    out = run(c, c.cov, c.sigma_px, c.fit_radius)
    dev = check_map(ref, c.cov, c.sigma_px, out, name)
    check_sums(ref, c.cov, c.sigma_px, out)
    return out, dev


def same_bits(a, b, scale=1.0):
    """every output of run a equals that of run b times `scale` bit for bit (NaN where NaN); M, G, n_fit and the flags equal"""
    eq = lambda x, y: np.array_equal(np.asarray(x) * scale, np.asarray(y), equal_nan=True)      # noqa: E731
    ok = eq(a["sigma"], b["sigma"]) and np.array_equal(a["flags"], b["flags"]) and np.array_equal(a["M"], b["M"]) and np.array_equal(a["G"], b["G"])
    ok = ok and a["n_fit"] == b["n_fit"] and all(a["summary"][k] == b["summary"][k] for k in ("count", "invalid", "worst"))
    ok = ok and eq(a["summary"]["sum_var"], b["summary"]["sum_var"]) and eq(a["summary"]["max_lam"], b["summary"]["max_lam"])
    for n in a["rings"]:
        ra, rb = a["rings"][n], b["rings"][n]
        ok = ok and np.array_equal(ra["count"], rb["count"]) and np.array_equal(ra["invalid"], rb["invalid"]) and eq(ra["sum_var"], rb["sum_var"]) and eq(ra["max_lam"], rb["max_lam"])
    return bool(ok)


# ------------------------------------------------------------------------------------------------------------ the semantic pin
# (model, parameter k, delta, max |d - J_k delta| in px from numpy at fit_radius 1 as the issue tabulates it)
PIN = (("poly3", 2, 0.1, 2.5e-5), ("poly3", 4, 1e-4, 3.5e-7), ("kb4", 3, 0.1, 1.9e-5), ("fov", 4, 1e-4, 1.4e-6), ("rational6", 0, 0.2, 2.1e-7))
PIN_FIT_RADIUS = 1.0


def rotation_vector(R):
    R = np.asarray(R)
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(v)
    return v if s < 1e-12 else v * (np.arcsin(min(s, 1.0)) / s)


def pin_cov(model, k, delta):
    cov = np.zeros((NK[model], NK[model]))
    cov[k, k] = delta * delta
    return cov


@functools.lru_cache(maxsize=None)
def pin_numpy(model, k, delta):
    """numpy's side of the pin: the comparer's difference map of K against K + delta e_k at the rotation fitted over the fit set by scipy
    (least_squares over rot(w)) -> (d [n, 2], w [3], the gap max |d - J_k delta| over the lattice)"""
    from scipy.optimize import least_squares
    ref = Reference(model, uc.gt(model), GRID, PIN_FIT_RADIUS)
    assert ref.valid.all()
    Kb = ref.K.copy(); Kb[k] += delta

    def diff(w, mask):
        return cc.project(model, Kb, ref.rays[mask] @ cc.rot(w).T) - ref.q[mask]
    sol = least_squares(lambda w: diff(w, ref.fit).ravel(), np.zeros(3), xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale=1e-3)
    d = diff(sol.x, np.ones(len(ref.q), dtype=bool))
    gap = float(np.linalg.norm(d - ref.J[:, :, k] * delta, axis=1).max())
    return d, sol.x, gap


def check_pin(model, k, delta, tabulated, out, d, w):
    """3. rank-one covariance delta^2 e_k e_k^T at sigma_px 1: sqrt(lam_s) against |d_s| of the difference map d (numpy's on the CPU, the real
    Comparer's on the GPU) within 1.5 x the numpy gap + 1e-7 px; M[:, k] delta against the fitted rotation's vector w within that bound over
    the smaller focal length (a rotation of that angle moves the centre pixel by the bound)"""
    _, _, gap = pin_numpy(model, k, delta)
    assert abs(gap - tabulated) <= 0.1 * tabulated, (model, k, gap, tabulated)
    bound = 1.5 * gap + 1e-7
    _, lam = var_lam(np.asarray(out["sigma"]).reshape(-1, 3))
    got = float(np.abs(np.sqrt(lam) - np.hypot(d[:, 0], d[:, 1])).max())
    K = uc.gt(model)
    got_w = float(np.abs(out["M"][:, k] * delta - np.asarray(w)).max())
    print("%s parameter %d: numpy gap %.3g px, |sqrt(lam) - |d|| %.3g px (bound %.3g), rotation off by %.3g rad (bound %.3g), largest |d| %.3g px" %
          (model, k, gap, got, bound, got_w, bound / min(K[0], K[1]), np.hypot(d[:, 0], d[:, 1]).max()))
    assert got <= bound
    assert got_w <= bound / min(K[0], K[1])
