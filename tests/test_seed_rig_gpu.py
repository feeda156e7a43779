"""The rig seed on the device (vc_seed_rig: one lane per candidate, the quadratic vote through LDS tiles, one wavefront per pair for the winner
and the refit) against the numpy reference (tests/seed_rig_ref.py), by the checks of tests/seed_rig_cases.py that tests/test_seed_rig_cpu.py
applies to the host build; the generator's 8-camera rig through the batched PnP and the Python face; the command line's -seed_rig mono."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import seed_rig_cases as sc
import seed_rig_ref as ref
import vicalib_amd.lib as lib
from vicalib_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")
ALL_CASES = [name for names in sc.GROUPS.values() for name in names]


@pytest.mark.parametrize("name", ALL_CASES)
def test_kernels_match_the_reference(name):
    sc.check(name, sc.device_seed_rig, label=" (device)")


def test_kernels_signs():
    sc.check_signs(sc.device_seed_rig, " (device)")


def test_kernels_bytes():
    sc.check_bytes(sc.device_seed_rig)


def test_empty_rigs():
    """no frame, one camera, nothing shared: statuses only, prefilled outputs untouched"""
    r = lib.seed_rig(np.zeros((0, 3), dtype=np.uint8), np.zeros((0, 3, 7)), out=sc.prefilled(3))
    assert list(r["pair_status"]) == [1, 1, 1] and list(r["pair_shared"]) == [0, 0, 0] and list(r["cam_status"]) == [0, 1, 1] and list(r["cam_parent"]) == [-1] * 3
    assert (r["pair_T_ab"] == sc.FILL_F).all() and (r["cam_T_c0"][1:] == sc.FILL_F).all() and list(r["cam_T_c0"][0]) == [0, 0, 0, 1, 0, 0, 0]
    c = sc.case("pair_3")
    r = lib.seed_rig(c["view_ok"][:, :1], c["view_T"][:, :1])
    assert r["pair_status"].size == 0 and list(r["cam_status"]) == [0] and list(r["cam_T_c0"][0]) == [0, 0, 0, 1, 0, 0, 0]
    assert lib.time_seed_rig(np.zeros((4, 2), dtype=np.uint8), np.full((4, 2, 7), np.nan), reps=2)["total"] == 0.0


# ------------------------------------------------------------------------------------------------ the generator's rig through the Python face
@functools.lru_cache(maxsize=None)
def rig8():
    return synth.generate(synth.Config(models=("fov", "kb4") * 4, n_frames=60, seed=5))


def _angle_deg(M):
    return float(np.rad2deg(np.arccos(max(-1.0, min(1.0, 0.5 * (np.trace(M[:3, :3]) - 1.0))))))


def truth_T_c0(p, c):
    return ref.pose_to_matrix(p.cam_T_ck_gt[c]) @ np.linalg.inv(ref.pose_to_matrix(p.cam_T_ck_gt[0]))


def test_pnp_poses_at_the_true_intrinsics_seed_the_eight_camera_rig():
    p = rig8()
    tiles = [t for t in p.tiles if len(t[2]) >= 4]
    off = np.concatenate([[0], np.cumsum([len(t[2]) for t in tiles])]).astype(np.int32)
    pw = np.concatenate([p.grid_points[t[2]] for t in tiles]); pc = np.concatenate([t[3] for t in tiles])
    pnp = lib.pnp_planar_batch([p.cam_model[t[1]] for t in tiles], [p.cam_K_gt[t[1]] for t in tiles], off, pw, pc)
    ok = np.zeros((60, 8), dtype=np.uint8); T = np.full((60, 8, 7), np.nan)
    for v, t in enumerate(tiles):
        if pnp["status"][v] == 0:
            ok[t[0], t[1]] = 1; T[t[0], t[1]] = pnp["T_cw"][v]
    r = lib.seed_rig(ok, T, tol_deg=3.0)
    assert (r["cam_status"] == 0).all() and (r["cam_parent"][1:] >= 0).all(), r
    for c in range(1, 8):
        d = ref.pose_to_matrix(r["cam_T_c0"][c]) @ np.linalg.inv(truth_T_c0(p, c))
        print("camera %d: %.4f degrees, %.2e m from the truth, parent %d" % (c, _angle_deg(d), np.linalg.norm(d[:3, 3]), r["cam_parent"][c]))
        assert _angle_deg(d) < 0.5, c
    # camera 7 against camera 0: one shared frame carries the planar pose ambiguity; it is outvoted and is not the winner
    pair = 6
    shared = np.nonzero(ok[:, 0] & ok[:, 7])[0]
    off_truth = [_angle_deg(ref.pose_to_matrix(T[k, 0]) @ np.linalg.inv(ref.pose_to_matrix(T[k, 7])) @ truth_T_c0(p, 7)) for k in shared]      # (X_k takes 7 into 0)
    flipped = [int(k) for k, a in zip(shared, off_truth) if a > 20.0]
    print("camera 7 against 0: %d shared, support %d, winner %d, flipped %s (%.1f degrees)" % (len(shared), r["pair_support"][pair], r["pair_winner"][pair], flipped, max(off_truth)))
    assert len(flipped) == 1 and r["pair_shared"][pair] == len(shared) and r["pair_support"][pair] == len(shared) - 1 and r["pair_winner"][pair] != flipped[0]
    t = lib.time_seed_rig(ok, T, tol_deg=3.0, reps=3)
    print("kernels:", t)
    assert t["candidates"] > 0.0 and t["support"] > 0.0 and t["finish"] > 0.0 and t["total"] > 0.0


# ------------------------------------------------------------------------------------------------ the command line
I_LINE = re.compile(r"^I -seed_rig: camera (\d+): parent (-?\d+), baseline (\S+) m, angle (\S+) degrees, support (\d+) / (\d+) shared frames, rms (\S+) degrees (\S+) m, "
                    r"T_c0 \[qx qy qz qw tx ty tz\] (\S+) (\S+) (\S+) (\S+) (\S+) (\S+) (\S+)$", re.M)


def test_cli_seed_rig_mono(tmp_path):
    """a 3-camera rig (poly3, fov, kb4) of 40 frames from identity poses: every camera is calibrated alone, cameras 1 and 2 are seeded within the
    seed's own tolerance of the truth (a seed further off than that found the wrong cluster), the run ends by itself; without the flag nothing
    of the seed appears"""
    p = synth.generate(synth.Config(models=("poly3", "fov", "kb4"), n_frames=40, seed=7))
    files, _ = synth.write_dataset(p, str(tmp_path))
    base = [BIN, "-cam", "detections://" + ",".join(files), "-models", "poly3,fov,kb4", "-nocalibrate_imu", "-grid_preset", "small", "-output", str(tmp_path / "cameras.xml")]
    r = subprocess.run(base + ["-seed_focal", "-pnp_device", "-seed_rig", "mono"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    print(r.stderr[-4000:]); print(r.stdout[-1500:])
    assert r.returncode in (0, 2), r.stdout + r.stderr
    alone = re.findall(r"^I -seed_rig: camera (\d+) alone: RMSE (\S+) px", r.stderr, re.M)
    assert [int(a[0]) for a in alone] == [0, 1, 2] and "W -seed_rig" not in r.stderr, r.stderr
    lines = I_LINE.findall(r.stderr)
    assert [int(m[0]) for m in lines] == [1, 2], r.stderr
    tol_deg = 3.0
    dist = float(np.median(np.linalg.norm(p.frame_T_wk_gt[:, 4:], axis=1)))          # camera 0 to the target's origin (the body is camera 0)
    for m in lines:
        c = int(m[0])
        T = np.array([float(x) for x in m[8:15]])
        truth = truth_T_c0(p, c)
        d = ref.pose_to_matrix(T) @ np.linalg.inv(truth)
        dt = float(np.linalg.norm(T[4:] - truth[:3, 3]))
        print("camera %d: %.3f degrees (of %g), %.4f m (of %.4f) from the truth" % (c, _angle_deg(d), tol_deg, dt, np.deg2rad(tol_deg) * dist))
        assert _angle_deg(d) <= tol_deg and dt <= np.deg2rad(tol_deg) * dist, (c, m)
        assert int(m[4]) >= 3 and int(m[4]) <= int(m[5]) <= 40
    plain = subprocess.run(base, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert "seed_rig" not in plain.stderr and plain.returncode in (0, 2), plain.stdout + plain.stderr


def test_cli_seed_rig_pnp_says_one_line_per_camera(tmp_path):
    """-seed_rig pnp at the default start intrinsics, the mode's documented weak case (its poses are biased there, so no accuracy is
    asserted): one PnP batch over the views of all cameras, then one I or W line for each of cameras 1 and 2, and the run ends by itself"""
    p = synth.generate(synth.Config(models=("poly3", "fov", "kb4"), n_frames=20, seed=7))
    files, _ = synth.write_dataset(p, str(tmp_path))
    r = subprocess.run([BIN, "-cam", "detections://" + ",".join(files), "-models", "poly3,fov,kb4", "-nocalibrate_imu", "-grid_preset", "small", "-max_iters", "5",
                        "-seed_rig", "pnp", "-output", str(tmp_path / "cameras.xml")], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    print(r.stderr[-3000:])
    assert r.returncode in (0, 2), r.stdout + r.stderr
    said = re.findall(r"^([IW]) -seed_rig: camera (\d+)(?: is not connected|: parent)", r.stderr, re.M)
    assert sorted(int(c) for _, c in said) == [1, 2] and "alone" not in r.stderr, r.stderr
    for m in I_LINE.findall(r.stderr):
        assert 3 <= int(m[4]) <= int(m[5]) <= 20 and np.isfinite([float(x) for x in m[8:15]]).all(), m


def test_cli_one_camera_has_nothing_to_seed(tmp_path):
    p = synth.generate(synth.Config(models=("poly3",), n_frames=12, seed=3))
    files, _ = synth.write_dataset(p, str(tmp_path))
    r = subprocess.run([BIN, "-cam", "detections://" + files[0], "-models", "poly3", "-nocalibrate_imu", "-grid_preset", "small", "-max_iters", "5", "-seed_rig", "pnp",
                        "-output", str(tmp_path / "cameras.xml")], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert "I -seed_rig: one camera, nothing to seed" in r.stderr and r.returncode in (0, 2), r.stdout + r.stderr
