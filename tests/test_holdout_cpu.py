"""What of the held-out scoring needs no device: the host reference of the per-frame problem (holdout_ref) against finite differences,
against a second start and on every case of the GPU tests; the command line's -holdout_every flag; the frame selection, compiled for the
host."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import holdout_cases as hc
import holdout_ref as hr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")


def _run(args):
    return subprocess.run([BIN] + args, capture_output=True, text=True, timeout=120)


# ------------------------------------------------------------------------------------------------ the host reference
@pytest.mark.parametrize("name", ["model-fov", "model-kb4", "model-rational6", "rig3"])
def test_reference_gradient_against_central_differences(name):
    """g = sum rho' J^T r of holdout_ref against central differences of its cost along T exp(h e_k): the truncation error of the
    difference is O(h^2 |f'''|), h = 1e-6 on costs of O(1e2..1e4) whose rounding noise is ~1e-16 * cost / h."""
    case = dict(hc.all_cases())[name]
    f = case["fitted"][0]
    fr = hc.ref_frame(case, f)
    T = case["seeds"][f]
    cost, g, H = fr.linearize(T)
    assert abs(cost - fr.cost(T)) <= 1e-14 * cost
    h = 1e-6
    fd = np.zeros(6)
    for k in range(6):
        e = np.zeros(6); e[k] = h
        fd[k] = (fr.cost(hr.se3_exp_apply(T, e)) - fr.cost(hr.se3_exp_apply(T, -e))) / (2 * h)
    err = np.abs(fd - g).max() / np.abs(g).max()
    print("%s: max |g| = %.3e, relative difference to central differences = %.3e" % (name, np.abs(g).max(), err))
    assert err <= 1e-6
    assert np.allclose(H, H.T) and np.all(np.linalg.eigvalsh(H) > 0)


def test_reference_converges_on_every_frame_of_every_case():
    """From the seeds the GPU tests use, to a gradient max-norm of 1e-12 times the one at the seed."""
    for name, case in hc.all_cases():
        ref = hc.reference(name)
        assert sorted(ref) == case["fitted"]
        for f, (T, info) in ref.items():
            assert info["converged"], (name, f, info)
            assert info["g"] <= 1e-12 * info["g0"]


@pytest.mark.parametrize("name", ["model-poly3", "rig2", "ragged"])
def test_reference_reaches_the_same_optimum_from_a_second_start(name):
    """The spread between two runs of the reference from different seeds: the level below which a comparison with it means something
    (the GPU tests hold the device to 1e-6 relative on the translation, 1e-6 rad on the rotation)."""
    case = dict(hc.all_cases())[name]
    worst_t = worst_r = 0.0
    for f in case["fitted"]:
        fr = hc.ref_frame(case, f)
        Ta, _ = hc.reference(name)[f]
        Tb, _ = hr.refine(fr, hc.perturbed(case["gt"][f], 500 + f, dt=0.004, dr=np.deg2rad(0.5)))
        dt, dr = hr.pose_distance(Ta, Tb)
        worst_t = max(worst_t, dt / np.linalg.norm(Ta[4:])); worst_r = max(worst_r, dr)
    print("%s: reference against reference from a second start: translation %.3e relative, rotation %.3e rad" % (name, worst_t, worst_r))
    assert worst_t <= 1e-7 and worst_r <= 1e-7


# ------------------------------------------------------------------------------------------------ the command line
def test_help_lists_holdout_every():
    h = _run(["--help"])
    assert h.returncode == 0 and "-holdout_every " in h.stdout


def test_holdout_every_is_checked_before_anything_is_read():
    for bad in ("1", "-3", "abc", "4x", ""):
        r = _run(["-cam", "detections:///does/not/exist.csv", "--holdout_every=" + bad])
        assert r.returncode == 1 and "holdout_every" in r.stderr and "cannot open" not in r.stderr, bad
    for good in ("0", "2", "5"):
        r = _run(["-cam", "detections:///does/not/exist.csv", "-holdout_every", good])
        assert r.returncode == 1 and "cannot open" in r.stderr, good           # got as far as the detections


def test_holdout_every_refuses_to_leave_fewer_than_two_fitting_frames(tmp_path):
    det = tmp_path / "cam0.csv"
    with open(det, "w") as f:
        for frame in range(3):
            for dot in range(4):
                f.write("%d,%d,%g,%g,%g,%g,0\n" % (frame, dot, 100.0 + 50 * dot, 100.0 + 30 * frame, 0.01 * dot, 0.01 * (dot % 2)))
    r = _run(["-cam", "detections://" + str(det), "-models", "poly3", "-holdout_every", "2", "-num_vicalib_frames", "2"])
    assert r.returncode == 1 and "holdout_every" in r.stderr and "fewer than 2" in r.stderr


# ------------------------------------------------------------------------------------------------ the frame selection
def _harness():
    src = os.path.join(HERE, "host_harness", "holdout_harness.cpp")
    so = os.path.join(HERE, "host_harness", "libvc_holdout_harness.so")
    dep = os.path.join(ROOT, "vicalib_amd", "csrc", "vc_holdout_select.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(dep)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = C.CDLL(so)
    L.vch_num_held.restype = C.c_longlong
    return L


def test_frame_selection_matches_its_statement():
    """Of the surviving frames 0, 1, 2, ... the last of every full group of N is held out; the count is n // N; N = 1, a negative N or
    fewer than two fitting frames are refused."""
    L = _harness()
    for every in (0, 2, 3, 4, 5, 7, 24, 25):
        for n in (0, 1, 2, 3, 4, 5, 23, 24, 25, 100):
            out = np.zeros(max(n, 1), dtype=np.int32)
            L.vch_held(C.c_longlong(n), every, out.ctypes.data_as(C.c_void_p))
            want = np.array([1 if every >= 2 and i % every == every - 1 else 0 for i in range(n)], dtype=np.int32)
            np.testing.assert_array_equal(out[:n], want)
            assert L.vch_num_held(C.c_longlong(n), every) == want.sum() == (n // every if every >= 2 else 0)
            assert L.vch_every_ok(C.c_longlong(n), every) == int(every == 0 or n - int(want.sum()) >= 2)
    assert L.vch_every_ok(C.c_longlong(100), 1) == 0 and L.vch_every_ok(C.c_longlong(100), -2) == 0
    assert L.vch_num_held(C.c_longlong(24), 4) == 6          # 24 frames, every 4th: 18 to fit, 6 to score
