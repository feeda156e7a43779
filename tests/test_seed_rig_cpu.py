"""The rig seed (vc_seed_rig), the part that needs no GPU: its arithmetic and its tree (vc_seed_rig.hpp) compiled for the host and run in plain
loops (tests/host_harness/seed_rig_harness.cpp), held to the numpy reference (tests/seed_rig_ref.py) by the checks of tests/seed_rig_cases.py,
the same checks tests/test_seed_rig_gpu.py applies to the kernels; the entry points' argument errors and their refusal to run without a
device; the Python face's refusals; the command line's flags."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import seed_rig_cases as sc
import vicalib_amd.lib as lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")
BAD_ARG, NO_DEVICE, UNSUPPORTED = -2, -1, -7
ALL_CASES = [name for names in sc.GROUPS.values() for name in names]


def _have_gpu():
    """(the device node first: where it exists torch is not asked -- a second HIP runtime initialised in this process after the library's
    has been seen to report no device on a machine that has one)"""
    if os.path.exists("/dev/kfd"):
        return True
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_the_cases_hold_what_they_claim():
    margins = sc.conditions()
    print("smallest relative distance of a comparison from a threshold:", min(margins.values()), min(margins, key=margins.get))
    k = sc.constants()
    assert k["max_cams"] == 8 and k["max_frames"] >= 65536 and k["tile"] == 256 and k["record"] == 8
    assert max(sc.PAIR_SIZES) > k["tile"] and {63, 64, 65} <= set(sc.PAIR_SIZES)          # the lane and the tile edges are among the sizes


@pytest.mark.parametrize("name", ALL_CASES)
def test_host_build_matches_the_reference(name):
    sc.check(name, sc.host_seed_rig, label=" (host build)")


def test_host_build_signs():
    sc.check_signs(sc.host_seed_rig, " (host build)")


def test_host_build_bytes():
    sc.check_bytes(sc.host_seed_rig)


# ---------------------------------------------------------------------------------------------- refusals
OUTS = ("pair_T_ab", "pair_shared", "pair_support", "pair_winner", "pair_rms_deg", "pair_rms_m", "pair_status", "cam_T_c0", "cam_parent", "cam_status")


def seed_rc(device=0, n_frames=None, n_cams=None, tol_deg=3.0, min_support=3, null=(), case="pair_3"):
    """the status of vc_seed_rig on a small rig with one thing wrong"""
    c = sc.case(case)
    ok, T = c["view_ok"], c["view_T"]
    o = sc.prefilled(max(ok.shape[1], n_cams or 0, 9))
    ptr = lambda k, a: None if k in null else sc._p(a)
    return lib.load().vc_seed_rig(device, ok.shape[0] if n_frames is None else n_frames, ok.shape[1] if n_cams is None else n_cams, ptr("view_ok", ok), ptr("view_T", T),
                                  C.c_double(tol_deg), min_support, *[ptr(k, o[k]) for k in OUTS])


def time_rc(device=0, reps=2, out=True, tol_deg=3.0, null=()):
    c = sc.case("pair_3")
    ms = np.zeros(3)
    ptr = lambda k, a: None if k in null else sc._p(a)
    return lib.load().vc_time_seed_rig(device, 3, 2, ptr("view_ok", c["view_ok"]), ptr("view_T", c["view_T"]), C.c_double(tol_deg), 3, reps, sc._p(ms) if out else None)


def test_argument_errors_come_before_the_device():
    for device in (0, -1):                                                   # (-1: no such device; the arguments are judged first)
        for missing in ("view_ok", "view_T") + OUTS:
            assert seed_rc(device=device, null=(missing,)) == BAD_ARG, missing
        assert seed_rc(device=device, n_frames=-1) == BAD_ARG and seed_rc(device=device, n_cams=0) == BAD_ARG and seed_rc(device=device, n_cams=-2) == BAD_ARG
        for tol in (0.0, -1.0, 90.0, 120.0, np.nan, np.inf):
            assert seed_rc(device=device, tol_deg=tol) == BAD_ARG, tol
            assert time_rc(device=device, tol_deg=tol) == BAD_ARG, tol
        assert seed_rc(device=device, min_support=0) == BAD_ARG and seed_rc(device=device, min_support=-3) == BAD_ARG
        assert seed_rc(device=device, n_cams=9) == UNSUPPORTED                  # (refused before anything behind the pointers is read)
        assert seed_rc(device=device, n_frames=sc.constants()["max_frames"] + 1) == UNSUPPORTED
        assert time_rc(device=device, reps=0) == BAD_ARG and time_rc(device=device, out=False) == BAD_ARG
        assert time_rc(device=device, null=("view_ok",)) == BAD_ARG and time_rc(device=device, null=("view_T",)) == BAD_ARG
    assert seed_rc(device=-1) == NO_DEVICE and time_rc(device=-1) == NO_DEVICE
    assert seed_rc(device=-1, n_frames=0) == NO_DEVICE and seed_rc(device=-1, n_cams=1) == NO_DEVICE      # (valid, if empty, rigs: no host fallback either)
    if not _have_gpu():          # no host fallback: a valid rig without a device is refused
        assert seed_rc() == NO_DEVICE and time_rc() == NO_DEVICE


def test_the_host_build_refuses_the_same_arguments():
    c = sc.case("pair_3")
    o = sc.prefilled(9)
    run = lambda nf, nc, tol, ms: sc.harness().seed_rig_harness_run(nf, nc, sc._p(c["view_ok"]), sc._p(c["view_T"]), C.c_double(tol), ms, *[sc._p(o[k]) for k in OUTS])
    assert run(3, 2, 3.0, 3) == 0
    assert run(-1, 2, 3.0, 3) == BAD_ARG and run(3, 0, 3.0, 3) == BAD_ARG and run(3, 2, 0.0, 3) == BAD_ARG and run(3, 2, 90.0, 3) == BAD_ARG and run(3, 2, 3.0, 0) == BAD_ARG
    assert run(3, 9, 3.0, 3) == UNSUPPORTED


def test_python_face_refuses_what_the_library_refuses():
    c = sc.case("pair_3")
    with pytest.raises(lib.VicalibError):
        lib.seed_rig(c["view_ok"], c["view_T"][:, :, :6])                     # not n x C x 7
    with pytest.raises(lib.VicalibError):
        lib.seed_rig(c["view_ok"][:-1], c["view_T"])                          # lengths disagree
    with pytest.raises(lib.VicalibError):
        lib.seed_rig(c["view_ok"][:, 0], c["view_T"][:, 0])                   # no camera axis
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        lib.seed_rig(c["view_ok"], c["view_T"], tol_deg=0.0)
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        lib.seed_rig(c["view_ok"], c["view_T"], min_support=0)
    with pytest.raises(lib.VicalibError, match="UNSUPPORTED"):
        lib.seed_rig(np.ones((3, 9), dtype=np.uint8), np.zeros((3, 9, 7)))
    if not _have_gpu():
        with pytest.raises(lib.VicalibError, match="NO_DEVICE"):
            lib.seed_rig(c["view_ok"], c["view_T"])
        with pytest.raises(lib.VicalibError, match="NO_DEVICE"):
            lib.time_seed_rig(c["view_ok"], c["view_T"])


def test_symbols_are_exported():
    assert "vc_seed_rig" in lib.SYMBOLS and "vc_time_seed_rig" in lib.SYMBOLS
    L = lib.load()
    assert L.vc_seed_rig and L.vc_time_seed_rig


# ---------------------------------------------------------------------------------------------- the command line
def test_help_lists_the_flags():
    r = subprocess.run([BIN, "-help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    for flag in ("-seed_rig ", "-seed_rig_tol_deg", "-seed_rig_min_support", "-seed_rig_max_rmse"):
        assert flag in text, flag
    assert "tens of degrees" in text                                          # the pnp mode's bias at the default start intrinsics is said


def test_flag_errors_exit_1_before_anything_is_read(tmp_path):
    """an unknown mode, -has_initial_guess beside the seed, a value out of range: exit status 1 and the flag's name, with or without a GPU,
    before the data set is opened (it does not exist)"""
    data = str(tmp_path / "no_such_data")
    base = [BIN, "-grid_preset", "small", "-cam", "detections://" + data + "/cam0.csv," + data + "/cam1.csv"]
    for extra in (["-seed_rig", "stereo"], ["-seed_rig", "PNP"],["-seed_rig", "pnp", "-has_initial_guess"], ["-seed_rig", "mono", "-has_initial_guess"],
                  ["-seed_rig", "pnp", "-seed_rig_tol_deg", "0"], ["-seed_rig", "pnp", "-seed_rig_tol_deg", "90"], ["-seed_rig", "mono", "-seed_rig_tol_deg", "nan"],
                  ["-seed_rig", "pnp", "-seed_rig_min_support", "0"], ["-seed_rig", "mono", "-seed_rig_max_rmse", "0"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
        assert r.returncode == 1 and r.stderr.startswith("ERROR:") and "seed_rig" in r.stderr, (extra, r.stdout + r.stderr)
