"""Depth registration (vc_regist*), the part that needs no GPU: the command line's flags and argument errors, the refusal to run without
a device, argument checks that come before the device, the conditions the cases must meet (from the reference alone), and the
kernels' arithmetic (vc_register.hpp) compiled for the host and held to the same checks against the numpy reference that
tests/test_register_gpu.py applies to the kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import register_cases as rc
import register_ref as rr
import undistort_cases as uc
import vicalib_amd.lib as lib
from vicalib_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")
FLAGS = ("-register_models", "-register_cams", "-register_depth", "-register_dir", "-register_unit", "-register_kind", "-register_splat", "-register_color",
         "-register_occlusion_tol")


def _have_gpu():
    """asked of the HIP runtime the library itself is linked against: what vc_registrar_create will see"""
    n = C.c_int(0)
    return lib.hip_runtime().hipGetDeviceCount(C.byref(n)) == 0 and n.value > 0


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _run(*args):
    return subprocess.run([BIN] + list(args), capture_output=True, text=True, timeout=60)


def rig_inputs(tmp_path, name="coarse", n=2, color=False):
    """an image case's cameras and the scene's first n depth images (and colour images) as files -> the tool's arguments"""
    cam_s, cam_d, kind, splat = rc.cameras(name)
    return rc.tool_inputs(tmp_path, cam_s, cam_d, kind, splat, rc.scene()[:n], rc.color_images(cam_d[2])[:n] if color else None)


# ------------------------------------------------------------------------------------------------------------ the tool
def test_cli_lists_the_register_flags():
    r = _run("-help")
    assert r.returncode == 0
    for flag in FLAGS:
        assert flag + " " in r.stdout, flag
    # the flags parse: the run gets as far as opening the rig file
    r = _run("-register_models", "/does/not/exist.xml", "-register_cams", "1,0", "-register_depth", "file:///does/not/exist_*.pgm", "-register_dir", "out",
             "-register_unit", "0.002", "-register_kind", "range", "-register_splat", "footprint", "-register_color", "file:///none_*.pgm", "-register_occlusion_tol", "3")
    assert r.returncode == 1 and "cannot open rig file" in r.stderr and "unknown command line flag" not in r.stderr


@pytest.mark.parametrize("args, message", [
    (["-register_kind", "depth"], "register_kind"),
    (["-register_splat", "bilinear"], "register_splat"),
    (["-register_unit", "0"], "register_unit"),
    (["-register_occlusion_tol", "-1"], "register_occlusion_tol"),
    (["-register_cams", "0"], "register_cams"),
    (["-register_cams", "0,2"], "register_cams"),
    (["-compare_models", "a.xml,b.xml", "-compare_dir", "cmp"], "exclude each other"),
    (["-convert_models", "a.xml", "-convert_to", "kb4"], "exclude each other"),
])
def test_cli_argument_errors(tmp_path, args, message):
    r = _run(*(rig_inputs(tmp_path) + args))
    assert r.returncode == 1 and message in r.stderr, r.stderr
    assert not (tmp_path / "out").exists()


def test_cli_needs_depth_and_dir(tmp_path):
    args = rig_inputs(tmp_path)
    r = _run(*args[:2])
    assert r.returncode == 1 and "-register_dir" in r.stderr


@pytest.mark.parametrize("other", [["-compare_models", "a.xml,b.xml", "-compare_dir", "cmp"], ["-convert_models", "a.xml", "-convert_to", "kb4"]], ids=["compare", "convert"])
def test_cli_register_depth_alone_excludes_the_file_modes(tmp_path, other):
    """without -register_models the registration waits for a calibration: a file-to-file mode beside it is refused, not run without it"""
    r = _run(*(rig_inputs(tmp_path)[2:] + other))
    assert r.returncode == 1 and "exclude each other" in r.stderr, r.stderr
    assert not (tmp_path / "out").exists()


def test_cli_refuses_a_header_larger_than_a_camera(tmp_path):
    args = rig_inputs(tmp_path, n=1)
    with open(tmp_path / "depth_00.pgm", "wb") as f:
        f.write(b"P5\n2000000 2000000\n65535\n\0\0")
    r = _run(*args)
    assert r.returncode == 1 and "8192 x 8192" in r.stderr, r.stderr
    assert not (tmp_path / "out").exists()


def test_cli_refuses_a_wrong_image_size_and_unequal_counts(tmp_path):
    args = rig_inputs(tmp_path, n=2, color=True)
    os.remove(tmp_path / "color_01.pgm")
    r = _run(*args)
    assert r.returncode == 1 and "2 files" in r.stderr and "1" in r.stderr, r.stderr
    rc.write_pgm8(tmp_path / "color_01.pgm", np.zeros((9, 9), dtype=np.uint8))
    r = _run(*args)
    assert r.returncode == 1 and "9 x 9 pixels" in r.stderr, r.stderr
    rc.write_pgm8(tmp_path / "depth_01.pgm", np.zeros((rc.SRC[1], rc.SRC[0]), dtype=np.uint8))          # an 8-bit file where a 16-bit one is expected
    r = _run(*args)
    assert r.returncode == 1 and "16-bit" in r.stderr, r.stderr
    assert not (tmp_path / "out").exists()


def test_cli_without_device(tmp_path):
    if _have_gpu():
        pytest.skip("GPU present")
    r = _run(*rig_inputs(tmp_path))
    assert r.returncode == 3 and "no HIP device" in r.stderr


# ------------------------------------------------------------------------------------------------------------ the library's checks
def _create(L, **kw):
    cam_s, cam_d, kind, splat = rc.cameras("coarse")
    a = dict(model_s=synth.MODEL_IDS[cam_s[0]], Ks=cam_s[1], nks=len(cam_s[1]), ws=cam_s[2][0], hs=cam_s[2][1], Ts=cam_s[3], model_d=synth.MODEL_IDS[cam_d[0]], Kd=cam_d[1],
             nkd=len(cam_d[1]), wd=cam_d[2][0], hd=cam_d[2][1], Td=cam_d[3], unit_src=0.001, unit_dst=0.001, kind=0, splat=0)
    a.update(kw)
    h = C.c_void_p()
    d = lambda x: None if x is None else _p(np.ascontiguousarray(x, dtype=np.float64))      # noqa: E731
    rc_ = L.vc_registrar_create(0, a["model_s"], d(a["Ks"]), a["nks"], a["ws"], a["hs"], d(a["Ts"]), a["model_d"], d(a["Kd"]), a["nkd"], a["wd"], a["hd"], d(a["Td"]),
                                C.c_double(a["unit_src"]), C.c_double(a["unit_dst"]), a["kind"], a["splat"], C.byref(h))
    return rc_, h


def test_no_cpu_fallback_without_device():
    if _have_gpu():
        pytest.skip("GPU present")
    L = lib.load()
    status, h = _create(L)
    assert status == -1 and not h.value                      # VC_ERR_NO_DEVICE
    cam_s, cam_d, kind, splat = rc.cameras("coarse")
    with pytest.raises(lib.VicalibError):
        lib.Registrar(cam_s, cam_d)


def test_arguments_are_checked_before_the_device():
    L = lib.load()
    long_q = rc.T_D.copy(); long_q[:4] *= 1.0 + 1e-5
    nan_t = rc.T_D.copy(); nan_t[5] = np.nan
    bad = [dict(model_s=9), dict(nks=6), dict(ws=1), dict(hs=8193), dict(model_d=-1), dict(nkd=4), dict(wd=8193), dict(hd=1), dict(Ts=long_q), dict(Td=nan_t),
           dict(Ts=None), dict(Ks=None), dict(unit_src=0.0), dict(unit_src=-0.001), dict(unit_dst=np.inf), dict(unit_dst=np.nan), dict(kind=2), dict(kind=-1),
           dict(splat=2), dict(splat=-1)]
    for kw in bad:
        status, h = _create(L, **kw)
        assert status == -2 and not h.value, kw              # VC_ERR_BAD_ARG, also where there is no device
    buf = np.zeros(64)
    assert L.vc_register_depth(None, 1, _p(buf), 4, C.c_longlong(4), _p(buf), 4, C.c_longlong(4), None, None) == -2
    assert L.vc_register_depth_device(None, 1, _p(buf), 4, C.c_longlong(4), _p(buf), 4, C.c_longlong(4), None, None) == -2
    assert L.vc_register_color(None, 1, _p(buf), 4, C.c_longlong(4), _p(buf), 4, C.c_longlong(4), C.c_double(0), 0, _p(buf), 4, C.c_longlong(4), None) == -2
    assert L.vc_register_points(None, 1, _p(buf), _p(buf), None) == -2 and L.vc_register_get(None, None, None, None, None, None, None, None) == -2
    assert L.vc_time_register(None, 1, 1, _p(buf)) == -2
    assert L.vc_registrar_create_for_cameras(None, 0, 1, C.c_double(0.001), C.c_double(0.001), 0, 0, C.byref(C.c_void_p())) == -2


# ------------------------------------------------------------------------------------------------------------ the cases, from the reference alone
@pytest.mark.parametrize("name", rc.IMAGE_CASES)
def test_cases_are_decided_and_under_the_cap(name):
    setup, tables, tests = rc.image_case(name)
    for t in tests:
        rc.assert_case_is_decided(setup, t)
        assert t["counters"][:7].sum() == rc.SRC[0] * rc.SRC[1]


def test_cases_meet_the_conditions():
    coarse = rc.image_case("coarse")[2][0]
    filled = coarse["hits"] > 0
    assert (coarse["distinct"] & filled).sum() >= 0.05 * filled.sum()          # more than one candidate with different w
    assert coarse["ties"].sum() >= 1                                           # equal w from different source pixels
    total = sum(t["counters"] for name in rc.IMAGE_CASES for t in rc.image_case(name)[2])
    assert np.all(total[:6] > 0), total                                        # every drop rule occurs
    near, foot = rc.image_case("fine_nearest")[2][0], rc.image_case("fine_footprint")[2][0]
    assert foot["counters"][7] >= 2 * near["counters"][7]
    assert (near["hits"] == 0).sum() > 0.5 * near["hits"].size                 # holes in nearest mode
    window = (slice(20, 50), slice(30, 100))                                   # inside the scene's image in D; it holds the foreground's shadow
    assert (foot["hits"][window] > 0).mean() > 0.85 and (near["hits"][window] > 0).mean() < 0.4          # a filled surface in footprint mode


@pytest.mark.parametrize("name, occl_tol", rc.GATHER_CASES)
def test_gather_cases_show_occlusion(name, occl_tol):
    col, refs = rc.gather_case(name, occl_tol)
    for ref in refs:
        n = ref["visible"].size
        assert 0.3 * n < ref["visible"].sum() < 0.95 * n
        assert (ref["passed"] & np.isfinite(ref["margin"]) & (ref["margin"] < 0)).sum() > 20          # occluded by a nearer surface


# ------------------------------------------------------------------------------------------------------------ the host build against the reference
def test_host_pose_relation():
    setup = rc.image_case("coarse")[0]
    g = rc.HostRegistrar(**rc.setup_args(setup), tables=False).get()
    np.testing.assert_allclose(g["R"], setup.R, rtol=0, atol=1e-15)
    np.testing.assert_allclose(g["t"], setup.t, rtol=0, atol=1e-15)


@pytest.mark.parametrize("case", rc.POINT_CASES, ids=lambda c: "%s-%s-%s" % (c[0], c[1], "range" if c[2] else "z"))
def test_host_points_against_the_reference(case):
    setup, rows, want, valid = rc.point_case(*case)
    got, ok = rc.HostRegistrar(**rc.setup_args(setup), tables=False).points(rows)
    d_px, d_w = rc.point_deviation(got, ok, want, valid)
    print("deviation of the host build: %.3g px, %.3g counts" % (d_px, d_w))
    assert d_px <= rc.D_PX and d_w <= rc.D_W, (d_px, d_w)


def test_host_points_invalid_rows():
    setup = rr.Setup(("poly3", rc.beyond_K(uc.FULL), uc.FULL, rc.T_S), ("poly3", uc.gt("poly3"), uc.FULL, rc.T_BEHIND), 0.001, 0.001, rr.KIND_Z, rr.NEAREST)
    rows = np.array([[320.0, 240.0, 1000.0],        # behind D
                     [2.0, 2.0, 1000.0],            # beyond S's image: no ray
                     [320.0, 240.0, 0.0], [320.0, 240.0, -5.0], [320.0, 240.0, np.nan], [320.0, 240.0, np.inf]])
    got, ok = rc.HostRegistrar(**rc.setup_args(setup), tables=False).points(rows)
    assert not ok.any() and np.isnan(got).all()


@pytest.mark.parametrize("name", rc.IMAGE_CASES)
def test_host_depth_against_the_reference(name):
    setup, tables, tests = rc.image_case(name)
    depth, index, counters = rc.HostRegistrar(**rc.setup_args(setup)).depth(rc.scene())
    for k, t in enumerate(tests):
        rc.check_depth(setup, t, depth[k], index[k], counters[k])


@pytest.mark.parametrize("name, occl_tol", rc.GATHER_CASES)
def test_host_gather_against_the_reference(name, occl_tol):
    setup, tables, tests = rc.image_case(name)
    col, refs = rc.gather_case(name, occl_tol)
    out, mask = rc.HostRegistrar(**rc.setup_args(setup)).color(rc.scene(), col, occl_tol, 7)
    for k, (t, ref) in enumerate(zip(tests, refs)):
        rc.check_gather(setup, t, ref, out[k], mask[k], 7)
