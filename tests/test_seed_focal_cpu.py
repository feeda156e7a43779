"""The focal-length seed (vc_seed_focal_batch), the part that needs no GPU: its arithmetic (vc_seed_focal.hpp) compiled for the host and run one
view and one camera at a time (tests/host_harness/seed_focal_harness.cpp), held to the numpy reference (tests/seed_focal_ref.py) by the checks
of tests/seed_focal_cases.py, the same checks tests/test_seed_focal_gpu.py applies to the kernels; the entry point's argument errors and its
refusal to run without a device; the Python face's refusals; the command line's flags."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import seed_focal_cases as sc
import seed_focal_ref as ref
import vicalib_amd.lib as lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")
BAD_ARG, NO_DEVICE = -2, -1


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_the_cases_cover_what_they_claim():
    b, spreads = sc.bound()                    # (asserts the statuses, the truth and the cap on the reference's output)
    assert set(spreads) == set(sc.GROUPS) and 0.0 < b <= 1e-6
    counts = sc.group("counts")
    assert [len(v["pw"]) for v in counts["views"][:8]] == sc.COUNTS
    assert np.isnan(counts["views"][8]["uv"]).sum() == 1 and len(set(counts["views"][9]["pw"][:, 2])) == 2
    models = sc.group("models")
    assert sorted({v["cam"] for v in models["views"]}) == list(range(6)) and [v["cam"] for v in models["views"][:7]] == [0, 1, 2, 3, 4, 5, 0]
    assert [len(sc.group(g)["pp"]) for g in ("counts", "truth", "radius", "cams", "models")] == [1, 2, 3, 4, 6]
    assert [v["cam"] for v in sc.group("cams")["views"]] == [0, 2, 0, 3, 2, 0, 0, 2, 0]
    assert sc.reference("fit_on")["view_status"].tolist() == [ref.OK, ref.BAD_FIT] and sc.reference("fit_off")["view_status"].tolist() == [ref.OK, ref.OK]
    assert all(len(sc.group(g)["views"]) == 40 for g in ("cap_fov", "cap_poly3", "cap_kb4"))


@pytest.mark.parametrize("name", sc.GROUPS)
def test_host_build_matches_the_reference(name):
    sc.check(name, sc.host_run(sc.group(name)), label=" (host build)")


def test_host_build_without_the_homographies():
    g = sc.group("counts")
    a, b = sc.host_run(g), sc.host_run(g, with_H=False)
    assert np.all(b["view_H"] == sc.FILL)
    for k in ("view_rows", "view_f", "view_fit_px", "view_used", "view_status", "cam_f", "cam_views", "cam_status"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_host_build_a_camera_does_not_depend_on_the_others():
    g = sc.group("cams")
    full = sc.host_run(g)
    own = [k for k, v in enumerate(g["views"]) if v["cam"] == 0]
    alone = sc.host_run(g, keep=own)
    assert alone["cam_f"][0].tobytes() == full["cam_f"][0].tobytes() and alone["cam_views"][0] == full["cam_views"][0] == 5
    assert alone["cam_status"].tolist() == [ref.CAM_OK, ref.CAM_NO_VIEW, ref.CAM_NO_VIEW, ref.CAM_NO_VIEW]


def test_min_corners_and_min_tilt_are_applied():
    """min_corners above a view's count refuses it; a min_tilt above every view's tilt refuses the camera and blanks the single-view estimates"""
    g = dict(sc.group("counts"), min_corners=64)
    got = sc.host_run(g)
    assert got["view_status"].tolist() == [ref.FEW] * 4 + [ref.FEW, ref.OK, ref.OK, ref.OK, ref.FEW, ref.NOT_PLANAR]
    steep = dict(sc.group("truth"), min_tilt=60.0)
    got, want = sc.host_run(steep), ref.batch(*sc.batch_arrays(steep), min_tilt_deg=60.0)
    assert np.array_equal(np.isnan(got["view_f"]), np.isnan(want["view_f"])) and np.isnan(got["view_f"]).any()
    assert np.isnan(got["view_f"]).sum() > np.isnan(sc.host_run(sc.group("truth"))["view_f"]).sum()
    assert got["cam_status"].tolist() == want["cam_status"].tolist()


def _call(n_views=2, n_cams=1, cam=None, pp=None, radius=True, off=None, pw=True, pc=True, max_fit=0.0, tilt=5.0, H=True, rows=True, f=True, fit=True, used=True,
          status=True, cam_f=True, cam_views=True, cam_status=True, device=0, use_cam=True, use_pp=True, use_off=True):
    L = lib.load()
    v = sc.group("counts")["views"][3]
    n = len(v["pw"])
    a = dict(cam=np.array([0, 0] if cam is None else cam, dtype=np.int32), pp=np.array([[320.0, 240.0]] * n_cams if pp is None else pp, dtype=np.float64),
             radius=np.zeros(max(n_cams, 1)), off=np.array([0, n, 2 * n] if off is None else off, dtype=np.int32), pw=np.concatenate([v["pw"]] * 2),
             pc=np.concatenate([v["uv"]] * 2), H=np.zeros((2, 9)), rows=np.zeros((2, 4)), f=np.zeros(2), fit=np.zeros(2), used=np.zeros(2, dtype=np.int32),
             status=np.zeros(2, dtype=np.int32), cam_f=np.zeros(max(n_cams, 1)), cam_views=np.zeros(max(n_cams, 1), dtype=np.int32),
             cam_status=np.zeros(max(n_cams, 1), dtype=np.int32))
    use = dict(cam=use_cam, pp=use_pp, radius=radius, off=use_off, pw=pw, pc=pc, H=H, rows=rows, f=f, fit=fit, used=used, status=status, cam_f=cam_f,
               cam_views=cam_views, cam_status=cam_status)
    p = {k: (sc._p(a[k]) if use[k] else None) for k in a}
    return L.vc_seed_focal_batch(device, n_views, p["cam"], n_cams, p["pp"], p["radius"], p["off"], p["pw"], p["pc"], 4, C.c_double(max_fit), C.c_double(tilt),
                                 p["H"], p["rows"], p["f"], p["fit"], p["used"], p["status"], p["cam_f"], p["cam_views"], p["cam_status"])


def test_argument_errors_come_before_the_device():
    for missing in ("use_cam", "use_pp", "radius", "use_off", "pw", "pc", "rows", "f", "fit", "used", "status", "cam_f", "cam_views", "cam_status"):
        assert _call(**{missing: False}) == BAD_ARG, missing
    assert _call(n_views=-1) == BAD_ARG
    assert _call(n_cams=0) == BAD_ARG and _call(n_cams=-3) == BAD_ARG
    assert _call(cam=[0, 1]) == BAD_ARG and _call(cam=[-1, 0]) == BAD_ARG and _call(n_cams=2, cam=[1, 2]) == BAD_ARG      # a view_cam outside 0 .. n_cams-1
    assert _call(off=[0, 8, 7]) == BAD_ARG and _call(off=[-1, 8, 16]) == BAD_ARG                                            # offsets that decrease; a negative start
    assert _call(pp=[[np.nan, 240.0]]) == BAD_ARG and _call(pp=[[320.0, np.inf]]) == BAD_ARG and _call(n_cams=2, pp=[[320.0, 240.0], [320.0, -np.inf]]) == BAD_ARG
    assert _call(max_fit=-0.5) == BAD_ARG and _call(max_fit=float("nan")) == BAD_ARG
    for tilt in (0.0, -5.0, 90.0, 120.0, float("nan")):
        assert _call(tilt=tilt) == BAD_ARG, tilt
    assert _call(device=-1, n_cams=0) == BAD_ARG                                                                            # (the arguments are judged before the device)
    L = lib.load()
    ms = C.c_double(0)
    v = sc.group("counts")["views"][3]
    a = [np.zeros(1, dtype=np.int32), np.array([320.0, 240.0]), np.zeros(1), np.array([0, len(v["pw"])], dtype=np.int32)]
    time = lambda reps, out, tilt=5.0: L.vc_time_seed_focal_batch(0, 1, sc._p(a[0]), 1, sc._p(a[1]), sc._p(a[2]), sc._p(a[3]), sc._p(v["pw"]), sc._p(v["uv"]), 4,
                                                                   C.c_double(0.0), C.c_double(tilt), reps, out)
    assert time(0, C.byref(ms)) == BAD_ARG and time(3, None) == BAD_ARG and time(3, C.byref(ms), tilt=95.0) == BAD_ARG
    if not _have_gpu():          # no host fallback: a valid call without a device is refused, the optional homographies asked for or not
        assert _call() == NO_DEVICE and _call(H=False) == NO_DEVICE and _call(n_views=0) == NO_DEVICE and time(3, C.byref(ms)) == NO_DEVICE


def test_python_face_refuses_what_the_library_refuses():
    cam, pp, rad, off, pw, uv = sc.batch_arrays(sc.group("truth"))
    with pytest.raises(lib.VicalibError):
        lib.seed_focal_batch(cam, pp, rad, off[:-1], pw, uv)                       # one offset short
    with pytest.raises(lib.VicalibError):
        lib.seed_focal_batch(cam, pp, rad[:1], off, pw, uv)                        # radii and principal points disagree
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        lib.seed_focal_batch(cam, pp, rad, off, pw, uv, min_tilt_deg=0.0)
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        lib.seed_focal_batch(cam + 1, pp, rad, off, pw, uv)
    if not _have_gpu():
        with pytest.raises(lib.VicalibError, match="NO_DEVICE"):
            lib.seed_focal_batch(cam, pp, rad, off, pw, uv)
        with pytest.raises(lib.VicalibError, match="NO_DEVICE"):
            lib.time_seed_focal_batch(cam, pp, rad, off, pw, uv, reps=2)


def test_help_lists_the_flags():
    r = subprocess.run([BIN, "-help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    for flag in ("-seed_focal ", "-seed_focal_radius", "-seed_focal_fit_px"):
        assert flag in text, flag


def test_seed_focal_with_model_files_is_a_flag_error(tmp_path):
    """refused before any device work: exit status 1 and the flags' names, with or without a GPU, and nothing written"""
    out = tmp_path / "cameras.xml"
    r = subprocess.run([BIN, "-cam", "detections://" + str(tmp_path / "none.csv"), "-model_files", str(tmp_path / "rig.xml"), "-seed_focal", "-output", str(out)],
                       capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == 1 and "-seed_focal" in r.stderr and "-model_files" in r.stderr, r.stdout + r.stderr
    assert not out.exists()
    r = subprocess.run([BIN, "-cam", "detections://" + str(tmp_path / "none.csv"), "-models", "poly3", "-seed_focal", "-seed_focal_fit_px", "-1", "-output", str(out)],
                       capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == 1 and "seed_focal_fit_px" in r.stderr, r.stdout + r.stderr
