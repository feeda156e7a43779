"""The focal-length seed on the device (vc_seed_focal_batch: one wavefront per view, then one per camera) against the numpy reference
(tests/seed_focal_ref.py), on the batches of tests/seed_focal_cases.py with that file's checks: statuses and counts exactly, H, the rows, the
fit and the focal lengths within 100 times the spread between the reference's two routes, the outputs of a refused view or camera untouched.
Determinism is compared on the raw bytes: a fixed reduction order promises the same bits for a view alone, among others and on a second run,
and for a camera whatever other cameras' views stand between its own.  Then the command line's -seed_focal.

test_cli_seed_focal measured (MI355X): see DESIGN 4.16."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import seed_focal_cases as sc
import seed_focal_ref as ref
import vicalib_amd.lib as lib
from vicalib_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")
VIEW_KEYS = ("view_status", "view_used", "view_H", "view_rows", "view_f", "view_fit_px")


def _run(g, keep=None):
    cam, pp, rad, off, pw, uv = sc.batch_arrays(g, keep)
    return lib.seed_focal_batch(cam, pp, rad, off, pw, uv, min_corners=g["min_corners"], max_fit_px=g["max_fit_px"], min_tilt_deg=sc.MIN_TILT,
                                out=sc.prefilled(len(cam), len(rad)))


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run(sc.group(name))
        return cache[name]
    return get


@pytest.mark.parametrize("name", sc.GROUPS)
def test_batch_matches_the_reference(runs, name):
    sc.check(name, runs(name), label=" (device)")


def test_refusal_statuses(runs):
    assert runs("counts")["view_status"].tolist() == [ref.FEW] + [ref.OK] * 8 + [ref.NOT_PLANAR]
    assert runs("radius")["view_status"].tolist() == [ref.FEW, ref.OK, ref.OK] and runs("radius")["view_used"][1] == 4
    assert runs("fit_on")["view_status"].tolist() == [ref.OK, ref.BAD_FIT] and runs("fit_off")["view_status"].tolist() == [ref.OK, ref.OK]
    assert runs("cams")["cam_status"].tolist() == [ref.CAM_OK, ref.CAM_NO_VIEW, ref.CAM_NO_TILT, ref.CAM_OK]
    assert runs("cams")["cam_views"].tolist() == [5, 0, 3, 1]


def _same_bits(a, b, rows_a, rows_b):
    for ka, kb in zip(rows_a, rows_b):
        for key in VIEW_KEYS:
            assert a[key][ka].tobytes() == b[key][kb].tobytes(), (key, ka, kb)


def test_a_view_gives_the_same_bits_alone_among_others_and_again(runs):
    """batches of 1, 4, 5 and 9 views: a lone wave, a full workgroup, a workgroup and one wave, two workgroups and one wave"""
    g = sc.group("counts")
    nine = _run(g, keep=range(9))
    _same_bits(nine, runs("counts"), range(9), range(9))                 # (the group's own run holds the same views first)
    _same_bits(nine, _run(g, keep=range(9)), range(9), range(9))
    for size in (1, 4, 5):
        _same_bits(_run(g, keep=range(size)), nine, range(size), range(size))
    for k in range(9):
        _same_bits(_run(g, keep=[k]), nine, [0], [k])


def test_a_camera_gives_the_same_bits_whatever_stands_between_its_views(runs):
    g = sc.group("cams")
    full = runs("cams")
    own = [k for k, v in enumerate(g["views"]) if v["cam"] == 0]
    for keep in (own, [k for k, v in enumerate(g["views"]) if v["cam"] in (0, 3)], range(9)):
        got = _run(g, keep=keep)
        assert got["cam_f"][0].tobytes() == full["cam_f"][0].tobytes() and got["cam_views"][0] == 5 and got["cam_status"][0] == ref.CAM_OK
    models = sc.group("models")
    full = runs("models")
    for c in (0, 5):
        got = _run(models, keep=[k for k, v in enumerate(models["views"]) if v["cam"] == c])
        assert got["cam_f"][c].tobytes() == full["cam_f"][c].tobytes()
        assert [s for k, s in enumerate(got["cam_status"]) if k != c] == [ref.CAM_NO_VIEW] * 5


def test_an_empty_batch_and_a_call_without_the_homographies(runs):
    g = sc.group("cams")
    empty = _run(g, keep=[])
    assert empty["cam_status"].tolist() == [ref.CAM_NO_VIEW] * 4 and empty["cam_views"].tolist() == [0] * 4 and np.all(empty["cam_f"] == sc.FILL)
    cam, pp, rad, off, pw, uv = sc.batch_arrays(g)
    n, nc = len(cam), len(rad)
    out = sc.prefilled(n, nc)
    status, cam_views, cam_status = np.zeros(n, dtype=np.int32), np.zeros(nc, dtype=np.int32), np.zeros(nc, dtype=np.int32)
    rc = lib.load().vc_seed_focal_batch(0, n, sc._p(cam), nc, sc._p(np.ascontiguousarray(pp)), sc._p(rad), sc._p(off), sc._p(pw), sc._p(uv), 4, C.c_double(0.0),
                                        C.c_double(sc.MIN_TILT), None, sc._p(out["view_rows"]), sc._p(out["view_f"]), sc._p(out["view_fit_px"]), sc._p(out["view_used"]),
                                        sc._p(status), sc._p(out["cam_f"]), sc._p(cam_views), sc._p(cam_status))
    assert rc == 0
    full = runs("cams")
    assert out["view_rows"].tobytes() == full["view_rows"].tobytes() and out["cam_f"].tobytes() == full["cam_f"].tobytes()
    assert status.tolist() == full["view_status"].tolist() and cam_status.tolist() == full["cam_status"].tolist()


def test_timing_hook_runs():
    cam, pp, rad, off, pw, uv = sc.batch_arrays(sc.group("models"))
    assert lib.time_seed_focal_batch(cam, pp, rad, off, pw, uv, reps=3) > 0.0


# ------------------------------------------------------------------------------------------------ the command line
CLI_K = (900.0, 900.0, 645.0, 477.0, -0.28, 0.09, -0.012)


def test_cli_seed_focal(tmp_path):
    """a poly3 camera of 1280 x 960 with f = 900 and the generator's distortion, principal point 5 px off the centre: with -seed_focal
    -pnp_device the calibration starts at the seeded focal length (inside the 25 % cap: the reference gives 943.9 on these detections) and ends
    like the other detection-file calibrations (the reprojection limit of 0.15 px behind "calibration succeeded", intrinsics to 3e-3)"""
    p = synth.generate(synth.Config(models=("poly3",), n_frames=40, seed=12, width=1280, height=960, gt_intrinsics=(CLI_K,)))
    files, _ = synth.write_dataset(p, str(tmp_path))
    out = tmp_path / "cameras.xml"
    base = [BIN, "-cam", "detections://" + files[0], "-models", "poly3", "-nocalibrate_imu", "-grid_preset", "small", "-image_width", "1280", "-image_height", "960",
            "-output", str(out)]
    r = subprocess.run(base + ["-seed_focal", "-pnp_device"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    print(r.stderr[-3000:])
    m = re.search(r"I camera 0: focal length seed ([0-9.]+) px from (\d+) of (\d+) views", r.stderr)
    assert m, r.stdout + r.stderr
    f, used, total = float(m.group(1)), int(m.group(2)), int(m.group(3))
    assert abs(f / 900.0 - 1.0) < 0.25 and used == total == 40
    assert r.returncode == 0, r.stdout + r.stderr
    assert "calibration succeeded" in r.stdout
    params = [float(x) for x in re.search(r"<params>\s*\[(.*?)\]", open(out).read(), re.S).group(1).split(";")]
    np.testing.assert_allclose(params[:4], CLI_K[:4], rtol=3e-3)
    # without the flag: no seed is computed or announced, and the run ends by itself as it did (from fx = fy = 300)
    plain = subprocess.run(base, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    print(plain.stderr[-1500:])
    assert "focal length seed" not in plain.stderr and plain.returncode in (0, 2), plain.stdout + plain.stderr
