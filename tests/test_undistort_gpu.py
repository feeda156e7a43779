"""Undistortion on the device (vc_undistort*, vicalib_amd/csrc/vc_undistort.hip): the lookup table against oracle_lib.project, the
bilinear remap against the rule evaluated in numpy from the stored table, the point inverse against the oracle's projection, the
fitted destination intrinsics, the command line, and the argument checks.  Cases and checks live in tests/undistort_cases.py (the
oracle's side is computed once per case); intrinsics are the synthetic generator's ground-truth values."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import undistort_cases as uc
import vicalib_amd.lib as lib
from vicalib_amd import synth
from vicalib_amd.lib import Undistorter

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")


# ---------------------------------------------------------------------------------------------------------------- 1. the map
@pytest.mark.parametrize("rot", ["identity", "rotated"])
@pytest.mark.parametrize("model", uc.MODELS)
def test_map_against_the_oracle(model, rot):
    uc.assert_profile_increasing(model)
    K, dl, R_ds, want, z = uc.map_case(model, rot)
    u = Undistorter(model, K, uc.SRC, dl, uc.DST, R_ds)
    m, valid = u.map()
    n_in, n_out = uc.check_map(model, uc.SRC, m, valid, want, z)
    assert n_in > 200 and n_out > 200, (n_in, n_out)
    got_dl, got_size = u.linear()
    assert np.array_equal(got_dl, dl) and got_size == uc.DST


def test_map_rays_behind_the_source_camera_are_invalid():
    K, dl, R_ds, src, want, z = uc.behind_case()
    m, valid = Undistorter("poly3", K, src, dl, uc.DST, R_ds).map()
    assert (z <= 0).sum() > 100 and valid.sum() > 100
    uc.check_map("poly3", src, m, valid, want, z)
    assert not valid[z <= 0].any()


# ---------------------------------------------------------------------------------------------------------------- 2. the remap
def _padded(n, size, pad, rng=None, value=None):
    """[n, h, w + pad] buffer and its [n, h, w] view"""
    buf = rng.integers(0, 256, (n, size[1], size[0] + pad), dtype=np.uint8) if rng is not None else np.full((n, size[1], size[0] + pad), value, dtype=np.uint8)
    return buf, buf[:, :, :size[0]]


@pytest.mark.parametrize("model,rot", [("poly3", "rotated"), ("kb4", "identity"), ("fov", "rotated")])
def test_remap_against_numpy(model, rot):
    K, dl, R_ds, _, _ = uc.map_case(model, rot)
    fill = 77
    u = Undistorter(model, K, uc.SRC, dl, uc.DST, R_ds, fill=fill)
    m, valid = u.map()
    assert valid.any() and (~valid).any()
    rng = np.random.default_rng(5)
    src_buf, src = _padded(3, uc.SRC, 5, rng=rng)                       # source pitch = width + 5
    dst_buf, dst = _padded(3, uc.DST, 3, value=201)                     # destination pitch = width + 3
    assert u.images(src, out=dst) is dst
    assert np.all(dst_buf[:, :, uc.DST[0]:] == 201)                     # the padding is the caller's
    n_half = uc.check_remap(dst, m, src, fill)
    print("%s %s: %d of %d pixels one grey level off at a half-integer" % (model, rot, n_half, dst.size))
    # the device entry point, same pitches, gives the same bytes
    d_src, d_dst = lib.DeviceBuffer(src_buf), lib.DeviceBuffer(np.full(dst_buf.shape, 201, dtype=np.uint8))
    u.images_device(3, d_src.ptr.value, src_buf.strides[1], src_buf.strides[0], d_dst.ptr.value, dst_buf.strides[1], dst_buf.strides[0])
    assert u.stream()
    assert np.array_equal(d_dst.numpy(), dst_buf)                       # (after a device-wide synchronisation)
    d_src.free(); d_dst.free()
    # one image, contiguous, through the same handle
    one = u.images(np.ascontiguousarray(src[1]))
    assert np.array_equal(one, dst[1])


def test_remap_identity_returns_the_image():
    """a linear source model equal to the destination model at the same size: bit for bit, x = w - 1 and y = h - 1 included"""
    K = np.array([61.7, 58.3, 26.3, 19.7])
    u = Undistorter("linear", K, uc.SRC, K, uc.SRC, fill=255)
    m, valid = u.map()
    assert valid.all()
    img = np.random.default_rng(6).integers(0, 256, (2, uc.SRC[1], uc.SRC[0]), dtype=np.uint8)
    assert np.array_equal(u.images(img), img)


# ---------------------------------------------------------------------------------------------------------------- 3. points
@pytest.mark.parametrize("model", uc.MODELS)
def test_points_round_trip(model):
    """Rays through the oracle into source pixels; vc_undistort_points returns the linear projection of the same rays to 1e-8 px: the stop
    rule leaves about 1e-14 in normalised units, times focal lengths below 500 and inverse profile slopes below 10 (asserted on the
    oracle's profile) -- three orders of margin.  Counts 1, 63, 64, 65 and 4096."""
    uc.assert_profile_increasing(model, max_inverse_slope=10.0)
    K, dl, R_ds, px, (want, front) = uc.point_case(model)
    assert max(K[0], K[1], dl[0], dl[1]) < 500
    u = Undistorter(model, K, uc.FULL, dl, uc.FULL, R_ds)
    for n in (1, 63, 64, 65, 4096):
        got, ok = u.points(px[:n])
        assert got.shape == (n, 2) and np.array_equal(ok, front[:n])
        err = np.abs(got[ok] - want[:n][ok]).max() if ok.any() else 0.0
        print("%s n = %d: max error %.3g px" % (model, n, err))
        assert err <= 1e-8
        assert np.isnan(got[~ok]).all()
    assert front.sum() > 4000


@pytest.mark.parametrize("model", uc.MODELS)
def test_points_keep_straight_lines_straight(model):
    K, lines = uc.line_case(model)
    _, dl, R_ds, _, _ = uc.point_case(model)
    u = Undistorter(model, K, uc.FULL, dl, uc.FULL, R_ds)
    for L in lines:
        assert uc.max_off_line(L) > 0.05 or model == "linear"         # (bent in the source image)
        q, ok = u.points(L)
        assert ok.all()
        off = uc.max_off_line(q)
        print("%s: %.3g px off the line" % (model, off))
        assert off <= 1e-8


def test_points_kb4_through_a_rotation():
    """kb4 with the rotation of (4, -7, 3) degrees: rays to 60 degrees off the axis, which stay in front of the rotated destination camera
    (1 + r_u^2 < 7 there, so the 1e-8 px of the round trip holds as for the other models)"""
    K, dl, R_ds, px, (want, front) = uc.kb4_rotated_point_case()
    assert front.all()
    u = Undistorter("kb4", K, uc.FULL, dl, uc.FULL, R_ds)
    got, ok = u.points(px)
    assert ok.all()
    err = np.abs(got - want).max()
    print("kb4 rotated: max error %.3g px" % err)
    assert err <= 1e-8


def test_points_beyond_the_models_image():
    K = uc.BEYOND_K
    r_max = 400.0 * 0.745356 * (1 - 0.6 * 0.745356 ** 2)             # 198.76 px: the profile's maximum
    phi = np.linspace(0, 2 * np.pi, 32, endpoint=False)
    dirs = np.stack([np.cos(phi), np.sin(phi)], 1)
    inside, beyond = K[2:4] + 0.9 * r_max * dirs, K[2:4] + np.linspace(1.01, 2.0, 32)[:, None] * r_max * dirs
    u = Undistorter("poly3", K, uc.FULL, [400.0, 400.0, 320.0, 240.0])
    q, ok = u.points(np.concatenate([inside, beyond]))
    assert ok[:32].all() and np.isfinite(q[:32]).all()
    assert not ok[32:].any() and np.isnan(q[32:]).all()


# ---------------------------------------------------------------------------------------------------------------- 4. fit_linear
@pytest.mark.parametrize("model", ["kb4", "poly3"])
def test_fit_linear(model):
    K = uc.gt(model); dst = (163, 121)
    u0 = Undistorter(model, K, uc.FULL, Undistorter.fit_linear(model, K, uc.FULL, dst, alpha=0.0), dst)
    assert u0.map()[1].all()                                          # alpha = 0: no invalid entry
    u1 = Undistorter(model, K, uc.FULL, Undistorter.fit_linear(model, K, uc.FULL, dst, alpha=1.0), dst)
    p, ok = u1.points(uc.border_samples(uc.FULL))                     # alpha = 1: every source border sample inside to 0.5 px
    assert ok.all()
    assert p[:, 0].min() >= -0.5 and p[:, 0].max() <= dst[0] - 0.5 and p[:, 1].min() >= -0.5 and p[:, 1].max() <= dst[1] - 0.5


# ---------------------------------------------------------------------------------------------------------------- 5. the command line
def _read_pgm(path):
    raw = open(path, "rb").read()
    m = re.match(rb"P5\s+(?:#[^\n]*\n\s*)*(\d+)\s+(\d+)\s+255\s", raw)
    w, h = int(m.group(1)), int(m.group(2))
    return np.frombuffer(raw[m.end():], dtype=np.uint8).reshape(h, w)


def test_cli_undistort_dir(tmp_path):
    """four rendered 160 x 120 views through -cam file://... -undistort_dir (flags as the image test of tests/test_cli.py)"""
    import dot_images
    pat = lib.target_make_pattern(6, 9, seed=71)
    views = [((0.3, -0.2, 0.1), 0.42), ((-0.35, 0.3, -0.3), 0.45), ((0.1, 0.4, 0.6), 0.40), ((-0.25, -0.35, 1.0), 0.44)]
    imgs = []
    for k, (tilt, dist) in enumerate(views):
        img, _ = dot_images.render(width=160, height=120, nx=9, ny=6, spacing=0.03, r_large=0.0094, r_small=0.0063, fu=140.0, fv=140.0, seed=k, tilt=tilt,
                                   dist=dist, pattern=pat, ss=4)
        imgs.append(img)
        with open(tmp_path / ("view_%03d.pgm" % k), "wb") as f:
            f.write(b"P5\n# rendered by tests/dot_images.py\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
            f.write(img.tobytes())
    out, und = tmp_path / "cameras.xml", tmp_path / "undistorted"
    args = ["-cam", "file://" + str(tmp_path / "view_*.pgm"), "-grid_height", "6", "-grid_width", "9", "-grid_spacing", "0.03", "-grid_seed", "71",
            "-models", "poly2", "-nocalibrate_imu", "-max_reprojection_error", "10", "-output", str(out)]
    r = subprocess.run([BIN] + args + ["-undistort_dir", str(und), "-undistort_alpha", "0.25"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "4 images" in r.stderr
    xml = lambda p: [float(x) for x in re.search(r"<params>\s*\[(.*?)\]", open(p).read(), re.S).group(1).split(";")]      # noqa: E731
    K = np.array(xml(out))
    assert len(K) == 6 and 'type="calibu_fu_fv_u0_v0_k1_k2"' in open(out).read()
    # cameras.xml of the directory: a linear model with the fitted intrinsics, the pose kept
    dl = Undistorter.fit_linear("poly2", K, (160, 120), alpha=0.25)
    txt = open(und / "cameras.xml").read()
    assert 'type="calibu_fu_fv_u0_v0"' in txt
    np.testing.assert_allclose(xml(und / "cameras.xml"), dl, rtol=1e-12)
    assert re.search(r"<T_wc>(.*?)</T_wc>", txt, re.S).group(1) == re.search(r"<T_wc>(.*?)</T_wc>", open(out).read(), re.S).group(1)
    # the images: at the source size, equal to Undistorter.images for the calibrated camera and the fitted intrinsics
    want = Undistorter("poly2", K, (160, 120), dl).images(np.stack(imgs))
    for k in range(4):
        got = _read_pgm(und / ("cam0_view_%03d.pgm" % k))
        assert got.shape == (120, 160) and np.array_equal(got, want[k])
    # detections:// input: a warning line, nothing written
    p = synth.generate(synth.Config(models=("poly3",), n_frames=12, seed=3))
    files, _ = synth.write_dataset(p, str(tmp_path))
    r = subprocess.run([BIN, "-cam", "detections://" + files[0], "-models", "poly3", "-nocalibrate_imu", "-output", str(tmp_path / "c2.xml"),
                        "-undistort_dir", str(tmp_path / "none")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "W -undistort_dir needs image input" in r.stderr and not (tmp_path / "none").exists()


# ---------------------------------------------------------------------------------------------------------------- 6. argument checks
def test_argument_checks():
    L = lib.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    K = uc.gt("poly3"); dl = np.array([400.0, 400.0, 320.0, 240.0]); h = C.c_void_p()
    create = lambda model, nk, w, R: L.vc_undistorter_create(0, model, p(K), nk, w, 480, p(dl), 640, 480, R, 0, C.byref(h))      # noqa: E731
    skew = np.eye(3); skew[0, 1] = 1e-6
    assert create(9, 7, 640, None) == -2                  # a bad model
    assert create(2, 6, 640, None) == -2                  # a wrong nparams
    assert create(2, 7, 1, None) == -2                    # a size of 1
    assert create(2, 7, 640, p(skew)) == -2               # not a rotation
    assert not h.value
    buf = np.zeros(16)
    assert L.vc_undistort_images(None, 1, p(buf), 4, C.c_longlong(16), p(buf), 4, C.c_longlong(16)) == -2
    assert L.vc_undistort_images_device(None, 1, p(buf), 4, C.c_longlong(16), p(buf), 4, C.c_longlong(16)) == -2
    assert L.vc_undistort_points(None, 1, p(buf), p(buf), None) == -2
    assert L.vc_undistort_get_map(None, None, None) == -2 and L.vc_undistort_get_linear(None, p(buf), None) == -2
    assert L.vc_time_undistort(None, 1, 1, p(buf)) == -2 and L.vc_undistort_stream(None) is None
    assert create(2, 7, 640, p(np.eye(3))) == 0           # ... and the same call with good arguments succeeds
    L.vc_undistorter_destroy(h)


def test_for_camera_and_timing_entry_point():
    """the handle made from a calibrator's camera is the handle made from the same numbers; vc_time_undistort returns three positive times"""
    from vicalib_amd.lib import ViCalibrator
    K = uc.gt("kb4")
    Ks = K.copy(); Ks[:4] *= 0.25
    dl = Undistorter.fit_linear("kb4", Ks, (160, 120), alpha=0.0)
    cal = ViCalibrator(0)
    cal.AddCamera("kb4", Ks, [0, 0, 0, 1, 0, 0, 0], 160, 120)
    a, b = Undistorter.for_camera(cal, 0, (160, 120), dl), Undistorter("kb4", Ks, (160, 120), dl)
    assert np.array_equal(a.map()[0], b.map()[0], equal_nan=True) and a.map()[1].all()
    t = a.time(n_images=3, reps=2)
    assert all(v > 0 for v in t.values()), t
