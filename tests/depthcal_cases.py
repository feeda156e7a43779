"""TEST INFRASTRUCTURE shared by test_depthcal_cpu.py and test_depthcal_gpu.py: the cases, the reference's side of every comparison
(depthcal_ref.py, computed once per case and kept), and the checks themselves -- written against an object with the interface of
vicalib_amd.lib.DepthCalibrator, so that the same check holds the host build of the kernels' arithmetic
(tests/host_harness/depthcal_harness.cpp) and the GPU kernels."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import depthcal_ref as dr        # noqa: E402
import register_cases as rc      # noqa: E402
from vicalib_amd import synth    # noqa: E402

SRC, BIG = rc.SRC, (131, 73)      # 67 x 35; 131 x 73: one cell of it holds more pixels than any one chunk of the accumulation
SRC_PITCH = 140                   # bytes: 2 * 67 + 6
RECT = (-0.6, -0.45, 0.6, 0.45)
UNIT, V_REF, MIN_COS, MAX_DEV = 0.001, 1000.0, 0.75, 60.0
MIN_COUNT, MIN_SPREAD = 100, 0.2  # of the fits the tests run: with them the range case shows all three cell statuses

# The host harness's largest deviation from the reference in y over all per-pixel cases, on used pixels (test_depthcal_cpu.py::
# test_host_expected_against_the_reference prints it), measured on the development machine, in counts.  The bound for host build and
# device alike is fifty times that: the margin the registrar and uncertainty tests give the device's FMA contraction over g++.
MEASURED_Y = 3.8e-10
D_Y = 50.0 * MEASURED_Y
# ... and its largest deviation from the numpy fit on identical sums (test_host_fit_against_the_reference prints it): coefficients, a, b
# and the RMS values, in counts
MEASURED_FIT = 3.5e-13
D_FIT = 50.0 * MEASURED_FIT
# v + delta is a sum of at most seven terms none of which exceeds 2^17 in these cases, each product and sum rounded once: two computations
# of it differ by less than 32 eps 2^17.  A pixel whose v + delta + 0.5 lies that close to an integer may round either way.
D_APPLY = 32.0 * dr.EPS * 131072.0
CAP = 0.02


def board_pose(height, tilt=(0.0, 0.0), spin=0.0, xy=(0.0, 0.0)):
    """T_wk of a rig `height` above the board's plane at xy, turned 180 degrees about x so that it looks at the board, then tilted and spun"""
    from scipy.spatial.transform import Rotation as R
    q = (R.from_euler("x", 180.0, degrees=True) * R.from_euler("xyz", (tilt[0], tilt[1], spin), degrees=True)).as_quat()
    return np.concatenate([q, [xy[0], xy[1], height]])


POSES = np.stack([
    board_pose(0.45), board_pose(0.60, (20.0, 0.0), 0.0, (0.05, 0.1)), board_pose(0.75, (0.0, -30.0), 0.0, (-0.2, 0.0)), board_pose(0.90, (35.0, 10.0), 0.0, (0.0, 0.25)),
    board_pose(1.05, (-50.0, 0.0), 0.0, (0.0, -0.5)), board_pose(1.20, (100.0, 0.0)), board_pose(1.35, (0.0, 0.0), 90.0), board_pose(1.50, (5.0, 25.0), 0.0, (0.3, 0.0))])
NOTHING = 5                       # the frame looking away: it contributes nothing
HELD_OUT = np.stack([board_pose(0.55, (10.0, -5.0), 20.0), board_pose(0.85, (-15.0, 20.0), -30.0, (0.1, 0.0)), board_pose(1.25, (25.0, 0.0), 45.0, (0.0, 0.1)),
                     board_pose(1.45, (0.0, -10.0), 10.0)])

# name -> (model, params, size, bins, unit, kind, v_ref, max_dev)
def _cases():
    p3 = rc.scaled_gt("poly3", SRC)
    out = {
        "main": ("poly3", p3, SRC, (4, 3), UNIT, dr.KIND_Z, V_REF, MAX_DEV),
        "range": ("kb4", rc.scaled_gt("kb4", SRC), SRC, (4, 3), UNIT, dr.KIND_RANGE, V_REF, MAX_DEV),
        "one": ("poly3", p3, SRC, (1, 1), UNIT, dr.KIND_Z, V_REF, MAX_DEV),
        "fine": ("poly3", p3, SRC, (32, 32), UNIT, dr.KIND_Z, V_REF, MAX_DEV),
        "beyond": ("poly3", rc.beyond_K(SRC), SRC, (4, 3), UNIT, dr.KIND_Z, V_REF, MAX_DEV),
        "small_unit": ("poly3", p3, SRC, (4, 3), 2e-5, dr.KIND_Z, 40000.0, 3000.0),
        "big_one": ("poly3", rc.scaled_gt("poly3", BIG), BIG, (1, 1), UNIT, dr.KIND_Z, V_REF, MAX_DEV),
        "big_two": ("poly3", rc.scaled_gt("poly3", BIG), BIG, (2, 1), UNIT, dr.KIND_Z, V_REF, MAX_DEV),
        "poly3_range": ("poly3", p3, SRC, (4, 3), UNIT, dr.KIND_RANGE, V_REF, MAX_DEV),
    }
    for m in rc.MODELS:
        if m != "poly3":
            out["z_" + m] = (m, rc.scaled_gt(m, SRC), SRC, (4, 3), UNIT, dr.KIND_Z, V_REF, MAX_DEV)
    return out


CASES = tuple(_cases())
SUM_CASES = ("main", "range", "one", "fine", "beyond", "small_unit", "big_one", "big_two")      # the others serve the per-pixel face only


@functools.lru_cache(maxsize=None)
def _rays(name_of_camera, kind):
    """the reference's inversion is a Python loop: once per camera and kind"""
    model, K, size = _cases()[name_of_camera][:3]
    return dr.Setup((model, K, size, rc.T_S), RECT, (1, 1), UNIT, kind, V_REF, MIN_COS, MAX_DEV).rays()


def _camera_key(name):
    model, K, size = _cases()[name][:3]
    for other in CASES:                                    # the first case with the same camera
        m, k, s = _cases()[other][:3]
        if m == model and s == size and np.array_equal(k, K):
            return other


def planted(setup, x, cells):
    """the error planted into the scenes, in counts: P(x) + a_cell + b_cell x"""
    a = 1.5 * np.sin(1.3 * np.arange(setup.cells) + 0.4); b = 3.0 * np.cos(0.9 * np.arange(setup.cells))
    return 8.0 + 12.0 * x - 10.0 * x * x + a[cells] + b[cells] * x


def render(setup, rays, has, poses):
    """Depth images [n, h, w] of the board seen from `poses`: the expected value minus the planted error (scaled to the case's v_ref),
    rounded; pixels that do not see the board get the value of their ray's intersection where there is one (else v_ref); then a band of
    zeros and a lattice of pixels raised by a fifth of v_ref (past the gate)."""
    w, h = setup.size
    cells = setup.cell_map().ravel()
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = np.zeros((len(poses), h, w), dtype=np.uint16)
    for k, T in enumerate(poses):
        y = dr.expected(setup, rays, has, T)["y"]
        y = np.where(np.isfinite(y), y, setup.v_ref)
        x = (y - setup.v_ref) / setup.v_ref
        v = np.rint(y - planted(setup, x, cells) * setup.v_ref / V_REF).reshape(h, w)
        v = np.where((ii % 9 == 4) & (jj % 7 == 3), v + 0.2 * setup.v_ref, v)
        v = np.clip(v, 1, 65535)
        v = np.where((jj >= 29 * h // 35) & (jj < 32 * h // 35), 0, v)
        out[k] = v
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(setup, rays, has, poses, depth, acc): acc is the reference's accumulation of all frames (depthcal_ref.accumulate)"""
    model, K, size, bins, unit, kind, v_ref, max_dev = _cases()[name]
    setup = dr.Setup((model, K, size, rc.T_S), RECT, bins, unit, kind, v_ref, MIN_COS, max_dev)
    rays, has = _rays(_camera_key(name), kind)
    depth = render(setup, rays, has, POSES)
    return dict(setup=setup, rays=rays, has=has, poses=POSES, depth=depth, acc=dr.accumulate(setup, rays, has, depth, POSES, D_Y))


@functools.lru_cache(maxsize=None)
def held_out(name):
    """frames that are not in the fit, at other poses: (depth [n, h, w], expected y [n, h w], rule [n, h w])"""
    c = case(name)
    depth = render(c["setup"], c["rays"], c["has"], HELD_OUT)
    ex = [dr.expected(c["setup"], c["rays"], c["has"], T, img) for T, img in zip(HELD_OUT, depth)]
    return depth, np.stack([e["y"] for e in ex]), np.stack([e["rule"] for e in ex])


def setup_args(setup):
    """the arguments of vicalib_amd.lib.DepthCalibrator"""
    return dict(cam=setup.cam, rect=setup.rect, bins=setup.bins, unit=setup.unit, kind=setup.kind, v_ref=setup.v_ref, min_cos=setup.min_cos, max_dev=setup.max_dev)


def strided(depth, pitch=None):
    """the images in a buffer whose rows are `pitch` bytes apart and whose images lie further apart than an image: (view [n, h, w], buffer)"""
    n, h, w = depth.shape
    pitch = pitch or 2 * w + 6
    stride = pitch * h + 64
    buf = np.full(n * stride, 0xAB, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf.view(np.uint16), shape=(n, h, w), strides=(stride, pitch, 2))
    view[...] = depth
    return view, buf


def padding_untouched(buf, n, h, w, pitch):
    stride = pitch * h + 64
    b = buf.reshape(n, stride)
    rows = b[:, :pitch * h].reshape(n, h, pitch)
    return bool(np.all(rows[:, :, 2 * w:] == 0xAB) and np.all(b[:, pitch * h:] == 0xAB))


# ------------------------------------------------------------------------------------------------------------ conditions on the cases
def assert_decided(c):
    """From the reference alone: no live pixel lies within D_Y of the gate or of the range limits, and no hit or incidence within 1e-9 of
    its threshold."""
    setup, acc = c["setup"], c["acc"]
    for k, T in enumerate(c["poses"]):
        ex = dr.expected(setup, c["rays"], c["has"], T, c["depth"][k])
        rule, y = ex["rule"], ex["y"]
        v = c["depth"][k].reshape(-1).astype(np.float64)
        with np.errstate(invalid="ignore"):
            assert not np.any((rule >= 3) & (np.abs(ex["edge"]) <= 1e-9))
            assert not np.any((rule >= 4) & (np.abs(ex["cosm"]) <= 1e-9))
            assert not np.any((rule >= 5) & ((np.abs(y - 1.0) <= D_Y) | (np.abs(y - 65535.0) <= D_Y)))
            assert not np.any((rule >= 6) & (np.abs(np.abs(y - v) - setup.max_dev) <= D_Y))
            assert not np.any((rule >= 2) & c["has"] & (np.abs(ex["s"]) < 1e-9))


# ------------------------------------------------------------------------------------------------------------ the checks
def check_expected(dc, c):
    """rule images exactly equal, with and without depth; y NaN exactly under rules 1 and 2.  Returns the largest deviation of y over the
    used pixels (of the call with depth) and over every pixel with a value (of the call without)."""
    setup = c["setup"]
    view, buf = strided(c["depth"], SRC_PITCH if setup.size == SRC else None)
    y, rule = dc.expected(c["poses"], view)
    y0, rule0 = dc.expected(c["poses"])
    n = len(c["poses"])
    worst = 0.0
    for k in range(n):
        ex = dr.expected(setup, c["rays"], c["has"], c["poses"][k], c["depth"][k])
        ex0 = dr.expected(setup, c["rays"], c["has"], c["poses"][k])
        assert np.array_equal(rule[k].ravel(), ex["rule"]), np.nonzero(rule[k].ravel() != ex["rule"])[0][:5]
        assert np.array_equal(rule0[k].ravel(), ex0["rule"])
        assert np.array_equal(np.isnan(y[k].ravel()), np.isnan(ex["y"])) and np.array_equal(np.isnan(y0[k].ravel()), np.isnan(ex0["y"]))
        used = ex["rule"] == 7
        if used.any():
            worst = max(worst, float(np.abs(y[k].ravel()[used] - ex["y"][used]).max()))
        inside = ex0["rule"] == 7
        if inside.any():
            worst = max(worst, float(np.abs(y0[k].ravel()[inside] - ex0["y"][inside]).max()))
    return worst


def add_all(dc, c, split=None, order=None):
    """the case's frames added in batches of `split` (default: one batch) in `order`; returns the counters [n, 8] in the order added"""
    order = list(range(len(c["poses"]))) if order is None else list(order)
    split = split or [len(order)]
    assert sum(split) == len(order)
    out, at = [], 0
    for m in split:
        idx = order[at:at + m]; at += m
        out.append(dc.add(c["depth"][idx], c["poses"][idx]))
    return np.concatenate(out)


def check_sums(dc, c):
    """counters exactly, sums within their derived bounds, totals against the column sums within the summation bound.  Returns the largest
    ratio of a sum's deviation to its bound."""
    acc = c["acc"]
    dc.clear()
    view, buf = strided(c["depth"])
    counters = dc.add(view, c["poses"])
    assert np.array_equal(counters, acc["counters"]), (counters, acc["counters"])
    s = dc.sums()
    assert np.array_equal(s["counters"], acc["counters"].sum(axis=0)) and s["n_frames"] == len(c["poses"])
    dev = np.abs(s["sums"] - acc["sums"])
    assert np.all(dev <= acc["bound"]), (np.argwhere(dev > acc["bound"])[:5], dev.max())
    col = s["sums"].sum(axis=0)
    assert np.all(np.abs(s["totals"] - col) <= c["setup"].cells * dr.EPS * np.abs(s["sums"]).sum(axis=0))
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.where(acc["bound"] > 0, dev / acc["bound"], 0.0)))


def bits(dc):
    s = dc.sums()
    return s["sums"].tobytes() + s["totals"].tobytes() + s["counters"].tobytes()


def check_reproducible(make, c):
    """two runs and two handles give the same bits; a batch of 8 equals 3 + 5 and eight single calls in the same frame order; clear followed
    by re-adding gives the same bits; a permuted frame order agrees within the bound"""
    a, b = make(c["setup"]), make(c["setup"])
    add_all(a, c); add_all(b, c)
    first = bits(a)
    assert bits(b) == first
    a.clear()
    assert not np.any(a.sums()["sums"]) and a.sums()["n_frames"] == 0 and not np.any(a.sums()["counters"])
    add_all(a, c, split=[3, 5])
    assert bits(a) == first
    a.clear(); add_all(a, c, split=[1] * 8)
    assert bits(a) == first
    a.clear(); add_all(a, c)
    assert bits(a) == first
    a.clear(); add_all(a, c, order=[6, 2, 7, 0, 5, 3, 1, 4])
    dev = np.abs(a.sums()["sums"] - b.sums()["sums"])
    assert np.all(dev <= 2.0 * c["acc"]["bound"])
    assert np.array_equal(a.sums()["counters"], b.sums()["counters"])


def fit_deviation(got, want):
    """statuses equal; the largest deviation over c, a, b and the three RMS values"""
    assert want is not None and np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    return float(max(np.abs(got["c"] - want["c"]).max(), np.abs(got["a"] - want["a"]).max(), np.abs(got["b"] - want["b"]).max(), np.abs(got["rms"] - want["rms"]).max()))


def check_fit(dc, c):
    """the fit of the handle's own sums against the reference's fit of the same sums, degrees 0, 1, 2.  Returns the largest deviation and
    the set of statuses met."""
    dc.clear(); add_all(dc, c)
    sums = dc.sums()["sums"]
    worst, seen = 0.0, set()
    for degree in (0, 1, 2):
        got = dc.fit(degree, MIN_COUNT, MIN_SPREAD)
        assert got["degree"] == degree and np.all(got["c"][degree + 1:] == 0)
        worst = max(worst, fit_deviation(got, dr.fit(sums, degree, MIN_COUNT, MIN_SPREAD)))
        seen |= set(int(s) for s in got["status"])
    return worst, seen


def undecided_rounding(ref):
    with np.errstate(invalid="ignore"):
        t = ref["sum"] + 0.5
        return np.abs(t - np.rint(t)) <= D_APPLY


def check_apply(make, c, degree=2):
    """the correction in both interpolation modes against the reference's image, exactly, outside the pixels whose rounding is undecided
    (at most CAP of them, asserted from the reference); set_fit(get_fit) on a fresh handle applies identically; in-place equals
    out-of-place and the padding is untouched.  Returns the number of excluded pixels."""
    setup = c["setup"]
    dc = make(setup)
    add_all(dc, c)
    f = dc.fit(degree, MIN_COUNT, MIN_SPREAD)
    fresh = make(setup)
    fresh.set_fit(f["degree"], f["c"], f["a"], f["b"])
    g = fresh.get_fit()
    assert np.array_equal(g["c"], f["c"]) and np.array_equal(g["a"], f["a"]) and np.array_equal(g["b"], f["b"]) and g["degree"] == f["degree"]
    excluded = 0
    n, h, w = c["depth"].shape
    for interp, code in (("cell", dr.CELL), ("bilinear", dr.BILINEAR)):
        out, counters = dc.apply(c["depth"], interp)
        out2, counters2 = fresh.apply(c["depth"], interp)
        assert np.array_equal(out, out2) and np.array_equal(counters, counters2)
        for k in range(n):
            ref = dr.correct(setup, f, c["depth"][k], code)
            skip = undecided_rounding(ref)
            assert skip.mean() <= CAP
            excluded += int(skip.sum())
            assert np.array_equal(out[k][~skip], ref["out"][~skip]), np.argwhere(~skip & (out[k] != ref["out"]))[:5]
            assert np.all(np.abs(counters[k] - ref["counters"]) <= skip.sum()) and counters[k].sum() == w * h
        view, buf = strided(c["depth"])
        pitch = 2 * w + 6
        same, counters3 = dc.apply(view, interp, out=view)                       # in place, strided
        assert np.array_equal(np.asarray(view), out) and np.array_equal(counters3, counters) and padding_untouched(buf, n, h, w, pitch)
    return excluded


def check_end_to_end(make, c, degree=2):
    """On frames that were not in the fit: the corrected images' raw RMS against the expected values is at most one fifth of the uncorrected
    one, over the pixels the rules keep.  Asserted first on the reference's own pipeline.  Returns (before, after, reference's after)."""
    setup = c["setup"]
    depth, y, rule = held_out_of(c)
    used = (rule == 7).reshape(depth.shape)
    yy = y.reshape(depth.shape)

    def rms(imgs):
        keep = used & (imgs != 0)
        return float(np.sqrt(np.mean((yy[keep] - imgs[keep].astype(np.float64)) ** 2)))
    before = rms(depth)
    fr = dr.fit(c["acc"]["sums"], degree, MIN_COUNT, MIN_SPREAD)
    after_ref = rms(np.stack([dr.correct(setup, fr, img, dr.BILINEAR)["out"] for img in depth]))
    assert used.sum() > 0.2 * used.size and after_ref <= before / 5.0, (before, after_ref)
    dc = make(setup)
    add_all(dc, c)
    dc.fit(degree, MIN_COUNT, MIN_SPREAD)
    out, _ = dc.apply(depth, "bilinear")
    after = rms(out)
    assert after <= before / 5.0, (before, after)
    return before, after, after_ref


def held_out_of(c):
    for name in CASES:
        if case(name) is c:
            return held_out(name)
    raise KeyError


# ------------------------------------------------------------------------------------------------------------ the host harness
def _harness():
    import ctypes as C
    import subprocess
    root = os.path.dirname(HERE)
    src = os.path.join(HERE, "host_harness", "depthcal_harness.cpp")
    so = os.path.join(HERE, "host_harness", "libvc_depthcal_harness.so")
    deps = [src] + [os.path.join(root, "vicalib_amd", "csrc", f) for f in ("vc_depthcal.hpp", "vc_register.hpp", "vc_report_bins.hpp", "vc_rectify.hpp", "vc_undistort.hpp",
                                                                            "vc_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = C.CDLL(so)
    L.dch_create.restype = C.c_void_p
    for name in ("dch_destroy", "dch_clear", "dch_sums", "dch_set_fit"):
        getattr(L, name).restype = None
    return L


class HostDepthCal:
    """vc_depthcal.hpp compiled with g++ behind the interface of vicalib_amd.lib.DepthCalibrator: one thread, pixels in row-major order"""

    def __init__(self, cam, rect, bins, unit, kind, v_ref, min_cos, max_dev):
        import ctypes as C
        self.C, self.L = C, _harness()
        m, K, size, T = cam
        d = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.c_void_p)      # noqa: E731
        self.h = C.c_void_p(self.L.dch_create(synth.MODEL_IDS[m], d(K), len(K), size[0], size[1], d(T), C.c_double(unit), int(kind), d(rect), int(bins[0]), int(bins[1]),
                                               C.c_double(v_ref), C.c_double(min_cos), C.c_double(max_dev)))
        assert self.h.value
        self.size, self.bins, self.cells = tuple(size), tuple(bins), bins[0] * bins[1]

    def __del__(self):
        if getattr(self, "h", None):
            self.L.dch_destroy(self.h)
            self.h = None

    def _p(self, x):
        return self.C.c_void_p(x.ctypes.data)

    def clear(self):
        self.L.dch_clear(self.h)

    def add(self, depth, T_wk):
        a = np.asarray(depth)
        if a.strides[2] != 2:
            a = np.ascontiguousarray(a)
        T = np.ascontiguousarray(T_wk, dtype=np.float64).reshape(-1, 7)
        n = len(a)
        cnt = np.zeros((n, 8), dtype=np.int64)
        assert self.L.dch_add(self.h, n, self._p(a), int(a.strides[1]), self.C.c_longlong(a.strides[0]), self._p(T), self._p(cnt)) == 0
        return cnt

    def expected(self, T_wk, depth=None):
        T = np.ascontiguousarray(T_wk, dtype=np.float64).reshape(-1, 7)
        n = len(T)
        y = np.zeros((n, self.size[1], self.size[0])); rule = np.zeros(y.shape, dtype=np.uint8)
        if depth is None:
            ptr, pitch, stride = None, 0, 0
        else:
            a = np.asarray(depth)
            ptr, pitch, stride = self._p(a), int(a.strides[1]), int(a.strides[0])
        assert self.L.dch_expected(self.h, n, self._p(T), ptr, pitch, self.C.c_longlong(stride), self._p(y), self._p(rule)) == 0
        return y, rule

    def sums(self):
        s = np.zeros((self.cells, 9)); tot = np.zeros(9); cnt = np.zeros(8, dtype=np.int64); nf = self.C.c_longlong(0)
        self.L.dch_sums(self.h, self._p(s), self._p(tot), self._p(cnt), self.C.byref(nf))
        return dict(sums=s, totals=tot, counters=cnt, n_frames=nf.value)

    def fit(self, degree=2, min_count=50, min_spread=0.02):
        rc_ = self.L.dch_fit(self.h, int(degree), int(min_count), self.C.c_double(min_spread))
        if rc_ != 0:
            raise ArithmeticError(rc_)
        return self.get_fit()

    def get_fit(self):
        c = np.zeros(3); a = np.zeros(self.cells); b = np.zeros(self.cells); st = np.zeros(self.cells, dtype=np.int32); rms = np.zeros(3); deg = self.C.c_int(0)
        if self.L.dch_get_fit(self.h, self._p(c), self._p(a), self._p(b), self._p(st), self._p(rms), self.C.byref(deg)) != 0:
            raise LookupError("no fit")
        return dict(c=c, a=a, b=b, status=st, rms=rms, degree=deg.value)

    def set_fit(self, degree, c, a, b):
        d = lambda x: np.ascontiguousarray(x, dtype=np.float64)      # noqa: E731
        c, a, b = d(c), d(a), d(b)
        self.L.dch_set_fit(self.h, int(degree), self._p(c), self._p(a), self._p(b))

    def apply(self, depth, interp="cell", out=None):
        a = np.asarray(depth)
        n = len(a)
        o = np.zeros((n, self.size[1], self.size[0]), dtype=np.uint16) if out is None else out
        cnt = np.zeros((n, 3), dtype=np.int64)
        ll = self.C.c_longlong
        assert self.L.dch_apply(self.h, n, self._p(a), int(a.strides[1]), ll(a.strides[0]), self._p(o), int(o.strides[1]), ll(o.strides[0]),
                                {"cell": 0, "bilinear": 1}[interp], self._p(cnt), None) == 0
        return o, cnt


def fit_sums_host(sums, degree, min_count, min_spread):
    """vc::dc_fit of any sums through the harness -> the dict of DepthCalibrator.get_fit, or None (VC_ERR_NUMERIC)"""
    import ctypes as C
    L = _harness()
    s = np.ascontiguousarray(sums, dtype=np.float64)
    cells = len(s)
    c = np.zeros(3); a = np.zeros(cells); b = np.zeros(cells); st = np.zeros(cells, dtype=np.int32); rms = np.zeros(3)
    p = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731
    if L.dch_fit_sums(p(s), cells, int(degree), int(min_count), C.c_double(min_spread), p(c), p(a), p(b), p(st), p(rms)) != 0:
        return None
    return dict(c=c, a=a, b=b, status=st, rms=rms, degree=degree)


def make_host(setup):
    return HostDepthCal(**setup_args(setup))


# ------------------------------------------------------------------------------------------------------------ files of the command-line tool
def poses_csv(poses):
    """the format -save_poses writes: two comment lines, then the top three rows of T_wk per line, ten digits"""
    out = ["% Pose file generated with vicalib.\n", "% Each line is the 12 elements from the top 3 rows of a 4x4transformation matrix, printed row major.\n"]
    for T in poses:
        R = dr.rr.quat_matrix(T[:4])
        out.append("     ".join(" ".join("%.10g" % x for x in list(R[r]) + [T[4 + r]]) for r in range(3)) + "\n")
    return "".join(out)


def tool_inputs(tmp_path, c, n=None):
    """rig.xml, poses.csv and the case's first n depth images as files -> the tool's arguments of the fit mode; the output goes to tmp_path/out"""
    setup = c["setup"]
    n = len(c["poses"]) if n is None else n
    with open(tmp_path / "rig.xml", "w") as f:
        f.write(rc.rig_xml([setup.cam]))
    with open(tmp_path / "poses.csv", "w") as f:
        f.write(poses_csv(c["poses"][:n]))
    for k in range(n):
        rc.write_pgm16(tmp_path / ("depth_%02d.pgm" % k), c["depth"][k])
    # (the tool's rectangle starts at the dot lattice's origin: TOOL_RECT, which tool_case moves the poses onto)
    return ["-depthcal_models", str(tmp_path / "rig.xml"), "-depthcal_cam", "0", "-depthcal_poses", str(tmp_path / "poses.csv"), "-depthcal_depth",
            "file://" + str(tmp_path / "depth_*.pgm"), "-depthcal_dir", str(tmp_path / "out"), "-depthcal_unit", repr(setup.unit), "-depthcal_kind",
            "range" if setup.kind else "z", "-depthcal_bins", "%d,%d" % setup.bins, "-depthcal_vref", repr(setup.v_ref), "-depthcal_min_cos", repr(setup.min_cos),
            "-depthcal_max_dev", repr(setup.max_dev), "-depthcal_degree", "2", "-depthcal_min_count", str(MIN_COUNT), "-depthcal_min_spread", repr(MIN_SPREAD),
            "-grid_width", "11", "-grid_height", "8", "-grid_spacing", "0.1", "-depthcal_margin", "0.1"]


TOOL_RECT = (-0.1, -0.1, 10 * 0.1 + 0.1, 7 * 0.1 + 0.1)       # what the tool makes of -grid_width 11 -grid_height 8 -grid_spacing 0.1 -depthcal_margin 0.1
TOOL_SHIFT = np.array([0.5, 0.35])        # the poses of the cases look at a board centred at the origin: the tool's is centred here


@functools.lru_cache(maxsize=None)
def tool_case(name="main"):
    """the case moved onto the tool's board: the same images, the poses shifted by TOOL_SHIFT in the target plane"""
    c = case(name)
    s = c["setup"]
    # (a rig file holds a pose as a matrix; the rotation of this one comes back from it to the bit, so that the tool and a handle made here
    # work with the same numbers)
    cam = (s.cam[0], s.cam[1], s.cam[2], np.array([0.0, 0.0, 0.0, 1.0, 0.02, -0.01, 0.03]))
    setup = dr.Setup(cam, TOOL_RECT, s.bins, s.unit, s.kind, s.v_ref, s.min_cos, s.max_dev)
    poses = c["poses"].copy(); poses[:, 4:6] += TOOL_SHIFT
    return dict(setup=setup, rays=c["rays"], has=c["has"], poses=poses, depth=c["depth"])


def g17(x):
    return "%.17g" % x


def correction_csv(setup, degree, f, sums):
    """depth_correction.csv as the tool writes it"""
    w, h = setup.size
    bx, by = setup.bins
    out = ["size,%d,%d" % (w, h), "bins,%d,%d" % (bx, by), "v_ref," + g17(setup.v_ref), "unit," + g17(setup.unit), "degree,%d" % degree,
           "c," + ",".join(g17(x) for x in f["c"]), "cx,cy,n,status,a,b"]
    for k in range(bx * by):
        out.append("%d,%d,%s,%d,%s,%s" % (k % bx, k // bx, g17(sums[k][0]), f["status"][k], g17(f["a"][k]), g17(f["b"][k])))
    return "\n".join(out) + "\n"


def cells_csv(setup, sums):
    bx = setup.bins[0]
    out = ["cx,cy,n,sum_x,sum_x2,sum_x3,sum_x4,sum_d,sum_dx,sum_dx2,sum_dd"]
    for k in range(len(sums)):
        out.append("%d,%d," % (k % bx, k // bx) + ",".join(g17(x) for x in sums[k]))
    return "\n".join(out) + "\n"


def read_frames_csv(path):
    """depthcal_frames.csv -> (names, counters [n, 8], poses [n, 7] as the tool parsed them)"""
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0] == "image,zero,no_ray,behind,outside,grazing,value_range,gate,used,qx,qy,qz,qw,tx,ty,tz"
    rows = [ln.split(",") for ln in lines[1:]]
    return [r[0] for r in rows], np.array([[int(x) for x in r[1:9]] for r in rows], dtype=np.int64), np.array([[float(x) for x in r[9:16]] for r in rows])


def read_correction_csv(path):
    with open(path) as f:
        lines = f.read().splitlines()
    head = {ln.split(",")[0]: ln.split(",")[1:] for ln in lines[:6]}
    rows = [ln.split(",") for ln in lines[7:]]
    return dict(degree=int(head["degree"][0]), c=np.array([float(x) for x in head["c"]]), a=np.array([float(r[4]) for r in rows]), b=np.array([float(r[5]) for r in rows]),
                status=np.array([int(r[3]) for r in rows]), bins=tuple(int(x) for x in head["bins"]), size=tuple(int(x) for x in head["size"]))


def read_rig_camera(path, index=0):
    """(params, T_ck) of camera `index` of a rig file in the layout of vc_write_camera_models: T_wc = [R_ck^T | -R_ck^T t_ck]"""
    import re
    from scipy.spatial.transform import Rotation as R
    with open(path) as f:
        text = f.read()
    cam = re.findall(r"<camera>.*?</camera>", text, re.S)[index]
    nums = lambda tag: [float(x) for x in re.split(r"[;,\s]+", re.search(r"<%s>\s*\[(.*?)\]\s*</%s>" % (tag, tag), cam, re.S).group(1).strip())]      # noqa: E731
    M = np.array(nums("T_wc")).reshape(3, 4)
    R_ck = M[:, :3].T
    return np.array(nums("params")), np.concatenate([R.from_matrix(R_ck).as_quat(), -R_ck @ M[:, 3]])


def read_pose_file(path):
    """[n, 7] from a file in the format -save_poses writes"""
    from scipy.spatial.transform import Rotation as R
    out = []
    with open(path) as f:
        for line in f:
            if line.strip() and not line.lstrip().startswith("%"):
                m = np.array([float(x) for x in line.split()]).reshape(3, 4)
                out.append(np.concatenate([R.from_matrix(m[:, :3]).as_quat(), m[:, 3]]))
    return np.array(out)


def read_cells_csv(path):
    with open(path) as f:
        return np.array([[float(x) for x in ln.split(",")[2:]] for ln in f.read().splitlines()[1:]])
