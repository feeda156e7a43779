"""Undistortion (vc_undistort*), the part that needs no GPU: the command line's flags, the refusal to run without a device, the host
fit of the destination intrinsics, and the kernels' arithmetic (vc_undistort.hpp) compiled for the host and held to the same checks
against the oracle that tests/test_undistort_gpu.py applies to the kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import undistort_cases as uc
import vicalib_amd.lib as lib
from vicalib_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _harness():
    src = os.path.join(HERE, "host_harness", "undistort_harness.cpp")
    so = os.path.join(HERE, "host_harness", "libvc_undistort_harness.so")
    deps = [src] + [os.path.join(ROOT, "vicalib_amd", "csrc", f) for f in ("vc_undistort.hpp", "vc_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_map(model, K, src, dl, dst, R_ds):
    m = np.zeros((dst[1], dst[0], 2), dtype=np.float32)
    R = np.ascontiguousarray(R_ds, dtype=np.float64)
    _harness().vuh_map(synth.MODEL_IDS[model], _p(K), len(K), src[0], src[1], _p(dl), dst[0], dst[1], _p(R), _p(m))
    return m, ~np.isnan(m[..., 0])


def host_points(model, K, dl, R_ds, px):
    px = np.ascontiguousarray(px, dtype=np.float64)
    out = np.zeros_like(px); valid = np.zeros(len(px), dtype=np.uint8)
    R = np.ascontiguousarray(R_ds, dtype=np.float64)
    _harness().vuh_points(synth.MODEL_IDS[model], _p(K), len(K), _p(dl), _p(R), len(px), _p(px), _p(out), _p(valid))
    return out, valid.astype(bool)


def test_cli_lists_the_undistort_flags():
    r = subprocess.run([BIN, "-help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for flag in ("-undistort_dir", "-undistort_alpha"):
        assert flag + " " in r.stdout, flag
    # the flags parse: the run gets as far as opening the detections
    r = subprocess.run([BIN, "-undistort_dir", "out", "-undistort_alpha", "0.5", "-cam", "detections:///does/not/exist.csv"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "cannot open" in r.stderr and "unknown command line flag" not in r.stderr


def test_no_cpu_fallback_without_device():
    if _have_gpu():
        pytest.skip("GPU present")
    L = lib.load()
    K = uc.gt("poly3"); dl = np.array([400.0, 400.0, 320.0, 240.0]); h = C.c_void_p()
    assert L.vc_undistorter_create(0, synth.MODEL_IDS["poly3"], _p(K), len(K), 640, 480, _p(dl), 640, 480, None, 0, C.byref(h)) == -1      # VC_ERR_NO_DEVICE
    assert not h.value
    with pytest.raises(lib.VicalibError):
        lib.Undistorter("poly3", K, (640, 480), dl)


def test_arguments_are_checked_before_the_device():
    L = lib.load()
    K = uc.gt("poly3"); dl = np.array([400.0, 400.0, 320.0, 240.0]); h = C.c_void_p()
    create = lambda model, nk, w, R: L.vc_undistorter_create(0, model, _p(K), nk, w, 480, _p(dl), 640, 480, R, 0, C.byref(h))      # noqa: E731
    skew = np.eye(3); skew[0, 1] = 1e-6
    assert create(9, 7, 640, None) == -2 and create(2, 6, 640, None) == -2 and create(2, 7, 1, None) == -2 and create(2, 7, 8193, None) == -2
    assert create(2, 7, 640, _p(skew)) == -2 and create(2, 7, 640, _p(-np.eye(3))) == -2
    assert L.vc_undistort_points(None, 1, _p(dl), _p(dl), None) == -2 and L.vc_undistort_get_map(None, None, None) == -2
    out = np.zeros(4)
    assert L.vc_undistort_fit_linear(2, _p(K), 7, 640, 480, 640, 480, C.c_double(1.5), _p(out)) == -2


@pytest.mark.parametrize("alpha", [0.0, 0.3, 1.0])
def test_fit_linear_returns_a_linear_camera_unchanged(alpha):
    K = np.array([411.25, 398.5, 317.75, 243.125])
    np.testing.assert_allclose(lib.Undistorter.fit_linear("linear", K, (640, 480), alpha=alpha), K, rtol=0, atol=1e-12)


@pytest.mark.parametrize("model", ["kb4", "poly3", "fov"])
def test_fit_linear_rectangles(model):
    """alpha = 0: every pixel of the destination border has a source pixel (the host build of the map's own test); alpha = 1: every
    sample of the source border lands inside the destination image to 0.5 px."""
    K = uc.gt(model); dst = (163, 121)
    dl0 = lib.Undistorter.fit_linear(model, K, uc.FULL, dst, alpha=0.0)
    m, valid = host_map(model, K, uc.FULL, dl0, dst, np.eye(3))
    assert valid.all()
    # ... and tightly: some border pixel of the destination lies within a source pixel of the source border
    edge = np.concatenate([m[0], m[-1], m[:, 0], m[:, -1]]).astype(np.float64)
    inside_by = np.minimum(np.minimum(edge[:, 0], uc.FULL[0] - 1 - edge[:, 0]), np.minimum(edge[:, 1], uc.FULL[1] - 1 - edge[:, 1]))
    assert inside_by.min() < 1.0
    dl1 = lib.Undistorter.fit_linear(model, K, uc.FULL, dst, alpha=1.0)
    p, ok = host_points(model, K, dl1, np.eye(3), uc.border_samples(uc.FULL))
    assert ok.all()
    assert p[:, 0].min() >= -0.5 and p[:, 0].max() <= dst[0] - 0.5 and p[:, 1].min() >= -0.5 and p[:, 1].max() <= dst[1] - 0.5
    dlh = lib.Undistorter.fit_linear(model, K, uc.FULL, dst, alpha=0.5)
    np.testing.assert_array_less(dl1[:2], dlh[:2]); np.testing.assert_array_less(dlh[:2], dl0[:2])      # focal lengths: wider view, shorter


@pytest.mark.parametrize("model", uc.MODELS)
def test_oracle_profiles_are_increasing(model):
    uc.assert_profile_increasing(model)


@pytest.mark.parametrize("rot", ["identity", "rotated"])
@pytest.mark.parametrize("model", uc.MODELS)
def test_host_map_against_the_oracle(model, rot):
    K, dl, R_ds, want, z = uc.map_case(model, rot)
    m, valid = host_map(model, K, uc.SRC, dl, uc.DST, R_ds)
    n_in, n_out = uc.check_map(model, uc.SRC, m, valid, want, z)
    assert n_in > 200 and n_out > 200, (n_in, n_out)          # the case exercises both


def test_host_map_behind_the_camera():
    K, dl, R_ds, src, want, z = uc.behind_case()
    m, valid = host_map("poly3", K, src, dl, uc.DST, R_ds)
    assert (z <= 0).sum() > 100 and valid.sum() > 100
    uc.check_map("poly3", src, m, valid, want, z)
    assert not valid[z <= 0].any()


@pytest.mark.parametrize("model", uc.MODELS)
def test_host_points_round_trip_and_straight_lines(model):
    uc.assert_profile_increasing(model)
    K, dl, R_ds, px, (want, front) = uc.point_case(model)
    got, ok = host_points(model, K, dl, R_ds, px)
    assert np.array_equal(ok, front) and front.sum() > 4000
    err = np.abs(got[front] - want[front]).max()
    assert err <= 1e-8, err
    K, lines = uc.line_case(model)
    for L in lines:
        q, ok = host_points(model, K, dl, R_ds, L)
        assert ok.all() and uc.max_off_line(q) <= 1e-8


def test_host_points_kb4_through_a_rotation():
    K, dl, R_ds, px, (want, front) = uc.kb4_rotated_point_case()
    got, ok = host_points("kb4", K, dl, R_ds, px)
    assert front.all() and ok.all()
    assert np.abs(got - want).max() <= 1e-8


def test_host_points_beyond_the_models_image():
    K = uc.BEYOND_K
    r_max = 400.0 * 0.745356 * (1 - 0.6 * 0.745356 ** 2)             # 198.76 px: the profile's maximum
    phi = np.linspace(0, 2 * np.pi, 32, endpoint=False)
    dirs = np.stack([np.cos(phi), np.sin(phi)], 1)
    inside, beyond = K[2:4] + 0.9 * r_max * dirs, K[2:4] + np.linspace(1.01, 2.0, 32)[:, None] * r_max * dirs
    dl = np.array([400.0, 400.0, 320.0, 240.0])
    q, ok = host_points("poly3", K, dl, np.eye(3), inside)
    assert ok.all() and np.isfinite(q).all()
    q, ok = host_points("poly3", K, dl, np.eye(3), beyond)
    assert not ok.any() and np.isnan(q).all()
