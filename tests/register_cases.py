"""TEST INFRASTRUCTURE shared by test_register_cpu.py and test_register_gpu.py: the cases, the reference's side of every comparison
(register_ref.py, computed once per case and kept), and the checks themselves -- written against plain arrays, so that the same check
holds the host build of the kernels' arithmetic (tests/host_harness/register_harness.cpp) and the GPU kernels."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import register_ref as rr        # noqa: E402
import undistort_cases as uc     # noqa: E402
from vicalib_amd import synth    # noqa: E402

MODELS = uc.MODELS
SRC = (67, 35)                    # neither a multiple of 64 nor of 4
COARSE, FINE = (45, 31), (131, 73)
SRC_PITCH = 2 * SRC[0] + 6        # bytes
BATCH = 3
UNIT_SRC, UNIT_DST = 0.001, 0.0005

# The harness's largest deviation from the reference over all point cases (test_register_cpu.py::test_host_points_against_the_reference
# prints it), measured on the development machine: pixels and values in D's unit.  The bound for harness and device alike is fifty times
# that -- the device build contracts to FMA where g++ does not, the margin the uncertainty tests use for the same situation.
MEASURED_PX, MEASURED_W = 2.7e-11, 3.9e-11
D_PX, D_W = 50.0 * MEASURED_PX, 50.0 * MEASURED_W
CAP = 0.02                        # at most this share of destination pixels / candidates may be excluded as ambiguous


def scaled_gt(model, size):
    """the synthetic ground-truth intrinsics of the 640 x 480 camera scaled to `size`"""
    K = uc.gt(model).copy()
    sx, sy = size[0] / uc.FULL[0], size[1] / uc.FULL[1]
    K[0] *= sx; K[2] *= sx; K[1] *= sy; K[3] *= sy
    return K


def pose(deg, t):
    """T_ck = [q (x y z w), t] of a camera turned by the Euler angles `deg` and shifted by t"""
    from scipy.spatial.transform import Rotation as R
    return np.concatenate([R.from_euler("xyz", deg, degrees=True).as_quat(), np.asarray(t, dtype=np.float64)])


T_S = pose((1.0, -2.0, 0.5), (0.02, -0.01, 0.03))
T_D = pose((-2.0, 3.0, -1.5), (0.12, 0.01, 0.02))              # about 0.1 m sideways and a few degrees against S
T_BEHIND = pose((0.0, 100.0, 0.0), (0.12, 0.01, 0.02))


def beyond_K(size):
    """poly3 whose profile r (1 - 0.7 r^2) has its maximum inside the image: the corners have no ray (and no pixel centre or lattice node
    lies within 4e-4 of that maximum, where an iterative inverse may or may not converge)"""
    K = uc.BEYOND_K.copy()
    K[4] = -0.7
    sx, sy = size[0] / uc.FULL[0], size[1] / uc.FULL[1]
    K[0] *= sx; K[2] *= sx; K[1] *= sy; K[3] *= sy
    return K


def zoomed(K, size, zoom):
    K = K.copy()
    K[0] *= zoom; K[1] *= zoom
    return K


# name -> (S model, S params, D model, D params, D size, T_D, kind, splat)
def _image_cases():
    s3 = scaled_gt("poly3", SRC)
    return {
        "coarse": ("poly3", s3, "fov", scaled_gt("fov", COARSE), COARSE, T_D, rr.KIND_Z, rr.NEAREST),
        "fine_nearest": ("poly3", s3, "rational6", scaled_gt("rational6", FINE), FINE, T_D, rr.KIND_Z, rr.NEAREST),
        "fine_footprint": ("poly3", s3, "rational6", scaled_gt("rational6", FINE), FINE, T_D, rr.KIND_Z, rr.FOOTPRINT),
        "range": ("kb4", scaled_gt("kb4", SRC), "poly3", scaled_gt("poly3", COARSE), COARSE, T_D, rr.KIND_RANGE, rr.NEAREST),
        "behind": ("poly3", s3, "poly3", scaled_gt("poly3", COARSE), COARSE, T_BEHIND, rr.KIND_Z, rr.NEAREST),
        "beyond": ("poly3", beyond_K(SRC), "poly3", scaled_gt("poly3", COARSE), COARSE, T_D, rr.KIND_Z, rr.FOOTPRINT),
        "zoom": ("poly3", s3, "poly2", zoomed(scaled_gt("poly2", FINE), FINE, 3.6), FINE, T_D, rr.KIND_Z, rr.FOOTPRINT),
    }


IMAGE_CASES = tuple(_image_cases())
GATHER_CASES = (("coarse", 0.0), ("fine_footprint", 2.5))


def scene():
    """BATCH depth images of SRC, uint16 [n, h, w]: a slanted background near 2 m, a foreground rectangle near 0.6 m, a band of zeros and
    a band of values so large that w exceeds 65535 in D's unit; the images differ by a shift of the foreground"""
    w, h = SRC
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = np.zeros((BATCH, h, w), dtype=np.uint16)
    for k in range(BATCH):
        d = 2000 + 3 * ii - 2 * jj + 7 * k
        fg = (ii >= 20 + 3 * k) & (ii < 41 + 3 * k) & (jj >= 8) & (jj < 23)
        d = np.where(fg, 600 + (ii % 5) + 2 * (jj % 3), d)
        d = np.where((jj >= 29) & (jj < 32), 0, d)
        d = np.where(ii >= 62, 50000 + 11 * jj, d)
        out[k] = d
    return out


def color_images(size):
    """BATCH 8-bit images of D: smooth and not symmetric"""
    w, h = size
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.stack([(128 + 100 * np.sin(0.21 * ii + 0.3 * k) * np.cos(0.17 * jj) + 20 * ((ii + 2 * jj) % 2)).astype(np.uint8) for k in range(BATCH)])


def cameras(name):
    ms, Ks, md, Kd, size_d, T_d, kind, splat = _image_cases()[name]
    return (ms, Ks, SRC, T_S), (md, Kd, size_d, T_d), kind, splat


@functools.lru_cache(maxsize=None)
def _tables(model_s, kind, beyond):
    K = beyond_K(SRC) if beyond else scaled_gt(model_s, SRC)
    setup = rr.Setup((model_s, K, SRC, T_S), (model_s, K, SRC, T_S), UNIT_SRC, UNIT_DST, kind, rr.NEAREST)
    return rr.Tables(setup)


@functools.lru_cache(maxsize=None)
def image_case(name):
    """(setup, tables, [depth_test of every image of the scene])"""
    cam_s, cam_d, kind, splat = cameras(name)
    setup = rr.Setup(cam_s, cam_d, UNIT_SRC, UNIT_DST, kind, splat)
    tables = _tables(cam_s[0], kind, name == "beyond")
    return setup, tables, [rr.depth_test(setup, tables, img) for img in scene()]


@functools.lru_cache(maxsize=None)
def gather_case(name, occl_tol, fill=7):
    setup, tables, tests = image_case(name)
    col = color_images(setup.cam_d[2])
    return col, [rr.gather(setup, tables, img, t, c, occl_tol, fill) for img, t, c in zip(scene(), tests, col)]


# ------------------------------------------------------------------------------------------------------------ ambiguity
def _near_integer(x, d):
    with np.errstate(invalid="ignore"):
        return np.abs(x - np.rint(x)) <= d


def ambiguity(setup, test):
    """(ambiguous [n_src] bool, excluded [h_d, w_d] bool): a source pixel that passed rules 0-2 in the reference is ambiguous when one
    of the numbers a floor acts on -- the rectangle's four edges (nearest: q + 0.5), m_d / unit_dst + 0.5 -- lies within D_PX / D_W of an
    integer; every destination pixel such a candidate can land on under either rounding is excluded."""
    wd, hd = setup.cam_d[2]
    has = test["code"] >= 3
    amb = has & (_near_integer(test["edges"], D_PX).any(axis=1) | _near_integer(test["warg"], D_W))
    excluded = np.zeros((hd, wd), dtype=bool)
    for e in np.nonzero(amb)[0]:
        x0, x1, y0, y1 = test["edges"][e]
        a, b = int(max(np.floor(x0 - D_PX), 0)), int(min(np.floor(x1 + D_PX), wd - 1))
        c, d = int(max(np.floor(y0 - D_PX), 0)), int(min(np.floor(y1 + D_PX), hd - 1))
        if a <= b and c <= d:
            excluded[c:d + 1, a:b + 1] = True
    return amb, excluded


def assert_case_is_decided(setup, test):
    """From the reference alone: no position hangs on the sign of z in D or on whether a ray exists (unproject asserts the latter), and the
    exclusion stays under the cap."""
    live = test["code"] >= 2
    assert np.all(np.abs(test["z_d"][live]) > 1e-6)
    amb, excluded = ambiguity(setup, test)
    n_cand = max(int((test["code"] >= 3).sum()), 1)
    assert excluded.mean() <= CAP and amb.sum() / n_cand <= CAP, (excluded.mean(), amb.sum() / n_cand)


def check_depth(setup, test, got_depth, got_index, got_counters):
    """Outside the excluded pixels depth and index agree exactly; every counter agrees to the number of ambiguous candidates.  Returns
    (excluded pixels, ambiguous candidates)."""
    amb, excluded = ambiguity(setup, test)
    keep = ~excluded
    got_depth = np.asarray(got_depth); got_index = np.asarray(got_index)
    assert got_depth.dtype == np.uint16 and got_index.dtype == np.int32
    assert np.array_equal(got_depth[keep], test["depth"][keep]), np.argwhere(keep & (got_depth != test["depth"]))[:5]
    assert np.array_equal(got_index[keep], test["index"][keep]), np.argwhere(keep & (got_index != test["index"]))[:5]
    diff = np.abs(np.asarray(got_counters, dtype=np.int64) - test["counters"])
    assert np.all(diff <= amb.sum()), (got_counters, test["counters"], int(amb.sum()))
    return int(excluded.sum()), int(amb.sum())


def gather_undecided(setup, test, ref):
    """[h_s, w_s] bool: the source pixels whose visibility the reference does not decide -- the border test within D_PX, a rounding of the
    pixel's own position or value within D_PX / D_W, a looked-up destination pixel that is excluded, or the comparison
    w <= w_win + occl_tol within D_W (both sides are integers plus occl_tol: an exact tie is decided)."""
    ws, hs = setup.cam_s[2]
    amb, excluded = ambiguity(setup, test)
    lookup = ref["lookup"]
    with np.errstate(invalid="ignore"):
        undecided = ref["passed"] & ((np.abs(ref["inside_by"]) <= D_PX) | _near_integer(ref["q"] + 0.5, D_PX).any(axis=1) | _near_integer(ref["warg"], D_W) |
                                     ((np.abs(ref["margin"]) <= D_W) & (ref["margin"] != 0)) | ((lookup >= 0) & excluded.ravel()[np.maximum(lookup, 0)]))
    return undecided.reshape(hs, ws)


def grey_undecided(ref):
    """[h_s, w_s] bool: the visible pixels whose unrounded bilinear value lies within 510 D_PX of a half-integer, so that two computations
    of it within D_PX of each other may round to different grey values"""
    return ref["visible"] & _near_integer(ref["value"] + 0.5, 510.0 * D_PX)


def check_gather(setup, test, ref, got, got_mask, fill):
    """The mask agrees wherever the reference is decided (gather_undecided); where both see the pixel its grey value lies within
    0.5 + 510 D_PX of the reference's unrounded bilinear value; everything else is `fill`.  Returns the number of undecided pixels."""
    undecided = gather_undecided(setup, test, ref)
    assert undecided.mean() <= CAP
    got = np.asarray(got); got_mask = np.asarray(got_mask, dtype=bool)
    assert np.array_equal(got_mask[~undecided], ref["visible"][~undecided]), np.argwhere(~undecided & (got_mask != ref["visible"]))[:5]
    assert np.all(got[~got_mask] == fill)
    both = got_mask & ref["visible"]
    err = np.abs(got[both].astype(np.float64) - ref["value"][both])
    assert np.all(err <= 0.5 + 510.0 * D_PX), err.max()
    return int(undecided.sum())


# ------------------------------------------------------------------------------------------------------------ points
POINT_CASES = tuple([(m, "poly3", k) for m in MODELS for k in (rr.KIND_Z, rr.KIND_RANGE)] + [("poly3", m, k) for m in MODELS if m != "poly3" for k in (rr.KIND_Z, rr.KIND_RANGE)])


@functools.lru_cache(maxsize=None)
def _source_pixels(model, n):
    """n rays over the model's field (kb4: to 60 degrees off the axis, so that every ray has an image in a destination turned by a few
    degrees) and their pixels in the full-size camera, through the oracle"""
    rng = np.random.default_rng(41 + synth.MODEL_IDS[model])
    t_max = np.radians(60.0) if model == "kb4" else uc.field_t_max(model)
    rays = uc.ray_at(model, t_max * np.sqrt(rng.uniform(0.0, 1.0, n)), rng.uniform(-np.pi, np.pi, n))
    return rays, uc.project(model, uc.gt(model), rays), rng.uniform(500.0, 4000.0, n)


@functools.lru_cache(maxsize=None)
def point_case(model_s, model_d, kind, n=4096):
    """(setup, rows (u, v, value) [n, 3], want (q_x, q_y, m_d / unit_dst) [n, 3], valid [n]): the rows are the oracle's pixels of known
    rays, the expectation is those rays at their distance through the oracle's projection of D -- no inverse on the reference's side"""
    rays, px, value = _source_pixels(model_s, n)
    setup = rr.Setup((model_s, uc.gt(model_s), uc.FULL, T_S), (model_d, uc.gt(model_d), uc.FULL, T_D), UNIT_SRC, UNIT_DST, kind, rr.NEAREST)
    q, wv, front, _ = setup.transfer(rays, value * UNIT_SRC)
    want = np.concatenate([q, wv[:, None]], axis=1)
    want[~front] = np.nan
    return setup, np.concatenate([px, value[:, None]], axis=1), want, front


def point_deviation(got, got_valid, want, valid):
    """(largest pixel deviation, largest value deviation) over the valid rows; validity agrees exactly and invalid rows are NaN"""
    got = np.asarray(got); got_valid = np.asarray(got_valid, dtype=bool)
    assert np.array_equal(got_valid, valid), np.nonzero(got_valid != valid)[0][:5]
    assert np.isnan(got[~valid]).all() and valid.sum() > 0.9 * len(valid)
    return float(np.abs(got[valid, :2] - want[valid, :2]).max()), float(np.abs(got[valid, 2] - want[valid, 2]).max())


def setup_args(setup):
    """the arguments of vicalib_amd.lib.Registrar"""
    return dict(cam_s=setup.cam_s, cam_d=setup.cam_d, unit_src=setup.unit_src, unit_dst=setup.unit_dst, kind=setup.kind, splat=setup.splat)


def strided_scene():
    """the scene in a buffer whose rows are SRC_PITCH bytes apart and whose images lie further apart than an image: (view [n, h, w], buffer)"""
    imgs = scene()
    w, h = SRC
    stride = SRC_PITCH * h + 64
    buf = np.full(BATCH * stride, 0xAB, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf.view(np.uint16), shape=(BATCH, h, w), strides=(stride, SRC_PITCH, 2))
    view[...] = imgs
    return view, buf


# ------------------------------------------------------------------------------------------------------------ the host harness
def _harness():
    import ctypes as C
    import subprocess
    root = os.path.dirname(HERE)
    src = os.path.join(HERE, "host_harness", "register_harness.cpp")
    so = os.path.join(HERE, "host_harness", "libvc_register_harness.so")
    deps = [src] + [os.path.join(root, "vicalib_amd", "csrc", f) for f in ("vc_register.hpp", "vc_rectify.hpp", "vc_undistort.hpp", "vc_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = C.CDLL(so)
    L.vrh_create.restype = C.c_void_p
    for name in ("vrh_destroy", "vrh_get", "vrh_depth", "vrh_color", "vrh_points"):
        getattr(L, name).restype = None
    return L


class HostRegistrar:
    """vc_register.hpp compiled with g++ behind the interface of vicalib_amd.lib.Registrar: one thread, a sequential scatter"""

    def __init__(self, cam_s, cam_d, unit_src, unit_dst, kind, splat, tables=True):
        import ctypes as C
        self.C, self.L = C, _harness()
        (ms, Ks, size_s, Ts), (md, Kd, size_d, Td) = cam_s, cam_d
        d = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.c_void_p)      # noqa: E731
        self.h = C.c_void_p(self.L.vrh_create(synth.MODEL_IDS[ms], d(Ks), len(Ks), size_s[0], size_s[1], d(Ts), synth.MODEL_IDS[md], d(Kd), len(Kd), size_d[0], size_d[1],
                                               d(Td), C.c_double(unit_src), C.c_double(unit_dst), int(kind), int(splat), int(tables)))
        assert self.h.value
        self.src_size, self.dst_size = tuple(size_s), tuple(size_d)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.vrh_destroy(self.h)
            self.h = None

    def get(self):
        R = np.zeros((3, 3)); t = np.zeros(3)
        self.L.vrh_get(self.h, R.ctypes.data_as(self.C.c_void_p), t.ctypes.data_as(self.C.c_void_p))
        return dict(R=R, t=t)

    def depth(self, arr, landed=None):
        """landed: an int64 array [n] that receives the number of key updates tried per image (what the kernel issues as atomics)"""
        C = self.C
        a = np.ascontiguousarray(arr, dtype=np.uint16)
        n = len(a)
        o = np.zeros((n, self.dst_size[1], self.dst_size[0]), dtype=np.uint16); idx = np.zeros(o.shape, dtype=np.int32); cnt = np.zeros((n, 8), dtype=np.int64)
        p = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731
        self.L.vrh_depth(self.h, n, p(a), int(a.strides[1]), C.c_longlong(a.strides[0]), p(o), int(o.strides[1]), C.c_longlong(o.strides[0]), p(idx), p(cnt),
                         None if landed is None else p(landed))
        return o, idx, cnt

    def color(self, depth, images, occl_tol=0.0, fill=0):
        C = self.C
        a = np.ascontiguousarray(depth, dtype=np.uint16); c = np.ascontiguousarray(images, dtype=np.uint8)
        n = len(a)
        o = np.zeros((n, self.src_size[1], self.src_size[0]), dtype=np.uint8); m = np.zeros_like(o)
        p = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731
        ll = C.c_longlong
        self.L.vrh_color(self.h, n, p(a), int(a.strides[1]), ll(a.strides[0]), p(c), int(c.strides[1]), ll(c.strides[0]), C.c_double(occl_tol), int(fill), p(o),
                         int(o.strides[1]), ll(o.strides[0]), p(m), None)
        return o, m.astype(bool)

    def points(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 3)
        out = np.zeros_like(rows); valid = np.zeros(len(rows), dtype=np.uint8)
        p = lambda x: self.C.c_void_p(x.ctypes.data)      # noqa: E731
        self.L.vrh_points(self.h, len(rows), p(rows), p(out), p(valid))
        return out, valid.astype(bool)


# ------------------------------------------------------------------------------------------------------------ files of the command-line tool
XML_TYPES = {"fov": "calibu_fu_fv_u0_v0_w", "poly2": "calibu_fu_fv_u0_v0_k1_k2", "poly3": "calibu_fu_fv_u0_v0_k1_k2_k3", "kb4": "calibu_fu_fv_u0_v0_kb4",
             "linear": "calibu_fu_fv_u0_v0", "rational6": "calibu_fu_fv_u0_v0_rational6"}


def rig_xml(cams):
    """a rig file in the layout of vc_write_camera_models, written here so that the CPU tests have one without a calibrator:
    cams = [(model, K, (w, h), T_ck)]; T_wc = [R_ck^T | -R_ck^T t_ck]"""
    out = ["<rig>"]
    vec = lambda v: "[ " + "; ".join("%.17g" % x for x in v) + " ]"      # noqa: E731
    for i, (m, K, size, T) in enumerate(cams):
        R = rr.quat_matrix(np.asarray(T[:4])); t = np.asarray(T[4:], dtype=np.float64)
        M, tw = R.T, -R.T @ t
        out += ["  <camera>", '    <camera_model name="" index="%d" serialno="-1" type="%s" version="8">' % (i, XML_TYPES[m]),
                "      <width> %d </width>" % size[0], "      <height> %d </height>" % size[1],
                "      <right> %s </right>" % vec([1, 0, 0]), "      <down> %s </down>" % vec([0, 1, 0]), "      <forward> %s </forward>" % vec([0, 0, 1]),
                "      <params> %s </params>" % vec(K), "    </camera_model>", "    <pose>",
                "      <T_wc> [ " + "; ".join(", ".join("%.17g" % x for x in list(M[r]) + [tw[r]]) for r in range(3)) + " ] </T_wc>", "    </pose>", "  </camera>"]
    return "\n".join(out + ["</rig>"]) + "\n"


def write_pgm16(path, img):
    """16-bit binary PGM, maxval 65535, most significant byte first"""
    img = np.asarray(img, dtype=np.uint16)
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n65535\n" % (img.shape[1], img.shape[0]))
        f.write(img.astype(">u2").tobytes())


def write_pgm8(path, img):
    img = np.asarray(img, dtype=np.uint8)
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())


def read_pgm(path):
    """a binary PGM of either depth -> uint8 or uint16 [h, w]"""
    with open(path, "rb") as f:
        data = f.read()
    magic, w, h, m = data.split(None, 4)[:4]
    assert magic == b"P5" and int(m) in (255, 65535)
    wide = int(m) > 255
    body = data[len(data) - int(w) * int(h) * (2 if wide else 1):]
    return np.frombuffer(body, dtype=">u2" if wide else np.uint8).reshape(int(h), int(w)).astype(np.uint16 if wide else np.uint8)


def tool_inputs(tmp_path, cam_s, cam_d, kind, splat, depth, color=None):
    """rig.xml, the depth images (and colour images) as files -> the tool's arguments; the output goes to tmp_path/out"""
    with open(tmp_path / "rig.xml", "w") as f:
        f.write(rig_xml([cam_s, cam_d]))
    for k, img in enumerate(depth):
        write_pgm16(tmp_path / ("depth_%02d.pgm" % k), img)
    args = ["-register_models", str(tmp_path / "rig.xml"), "-register_depth", "file://" + str(tmp_path / "depth_*.pgm"), "-register_dir", str(tmp_path / "out"),
            "-register_kind", "range" if kind else "z", "-register_splat", "footprint" if splat else "nearest"]
    if color is not None:
        for k, img in enumerate(color):
            write_pgm8(tmp_path / ("color_%02d.pgm" % k), img)
        args += ["-register_color", "file://" + str(tmp_path / "color_*.pgm")]
    return args
