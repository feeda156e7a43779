"""The target step (vc_target_refine_batch), the part that needs no GPU: its arithmetic (vc_target_refine.hpp) compiled for the host
(tests/host_harness/target_refine_harness.cpp) and held to the numpy reference of tests/target_refine_ref.py by the checks of
tests/target_refine_cases.py -- the same checks tests/test_target_refine_gpu.py applies to the kernels --, the properties of the definition, the
argument errors of the C ABI (which come before any device call) and its refusal to run without a device."""
import ctypes as C

import numpy as np
import pytest

import select_cases as sc
import target_refine_cases as tc
import target_refine_ref as ref
import vicalib_amd.lib as lib


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(name):
        if name not in cache:
            rc, out = tc.host_step(tc.cases()[name])
            assert rc == 0
            cache[name] = out
        return cache[name]
    return get


@pytest.mark.parametrize("name", tc.NAMES)
def test_step_matches_reference(runs, name):
    tc.check(name, runs(name), " (host)")


def test_exact_measurements_give_no_step(runs):
    got, case = runs("exact"), tc.cases()["exact"]
    b = tc.bounds("exact")[0]["refined"]
    assert np.abs(got["refined"] - case["nominal"]).max() <= b


def test_similarity_in_points_changes_nothing(runs):
    """on the exact case (tests/test_target_refine_cases_cpu.py says why there)"""
    rc, moved = tc.host_step(tc.moved_by_small_similarity("exact"))
    assert rc == 0
    assert np.abs(moved["refined"] - runs("exact")["refined"]).max() <= tc.bounds("exact")[0]["refined"]


def test_similarity_in_points_with_a_real_step(runs):
    """a noisy case, d != 0: `refined` moves by no more than the step turns with the board (tc.similarity_bound), some 50 times less than the similarity"""
    name = "mono_poly3"
    moved = tc.host_step(tc.moved_by_small_similarity("mono_poly3"))[1]
    shift = np.abs(moved["refined"] - runs(name)["refined"]).max()
    delta = np.abs(tc.moved_by_small_similarity(name)["points"] - tc.cases()[name]["points"]).max()
    print("similarity %.3e m moves refined by %.3e m, bound %.3e m" % (delta, shift, tc.similarity_bound(name)))
    assert delta >= 20.0 * tc.similarity_bound(name)
    assert shift <= tc.similarity_bound(name)


def test_unobserved_rows_keep_their_bits(runs):
    got, case = runs("mixed"), tc.cases()["mixed"]
    sp = case["special"]
    for p in (sp["never"], sp["behind"]):
        assert got["point_status"][p] == 1 and got["refined"][p].tobytes() == np.asarray(case["points"][p], dtype=np.float64).tobytes()
    assert got["refined"][sp["never"]].tolist() != case["nominal"][sp["never"]].tolist()


def test_unsupported_and_bad_arguments_of_the_host_build():
    assert tc.host_step(tc.unsupported_case())[0] == -7
    small = dict(tc.cases()["p4_n1_fixed"]); small["points"] = small["points"][:3]; small["nominal"] = small["nominal"][:3]
    small["tiles"] = [(f, c, ids[:3] % 3, z[:3]) for f, c, ids, z in small["tiles"]]
    assert tc.host_step(small)[0] == -2
    bad = dict(tc.cases()["p21_n5"]); bad["lam"] = 0.0
    assert tc.host_step(bad)[0] == -2


# ---------------------------------------------------------------------------------------------- the C ABI without a device
def test_symbols_are_exported():
    L = lib.load()
    assert hasattr(L, "vc_target_refine_batch") and hasattr(L, "vc_time_target_refine_batch")
    assert "vc_target_refine_batch" in lib.SYMBOLS and "vc_time_target_refine_batch" in lib.SYMBOLS


def _call(case, device=0, **change):
    a = tc.lib_args(case)
    a.update(change)
    return lib.target_refine_batch(device=device, **a)


def _rc(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except lib.VicalibError as e:
        return str(e)
    return ""


def test_argument_errors_come_before_the_device():
    """a device that does not exist (99): every bad argument is still VC_ERR_BAD_ARG / VC_ERR_UNSUPPORTED, not VC_ERR_NO_DEVICE"""
    case = tc.cases()["p21_n5"]
    a = tc.lib_args(case)
    pid = a["point_id"].copy(); pid[5] = 21
    off = a["tile_off"].copy(); off[2] = off[1] - 1
    tf = a["tile_frame"].copy(); tf[0] = 5
    tcam = a["tile_cam"].copy(); tcam[0] = 1
    m, K, T, fl = case["cameras"][0]
    for change, code in ((dict(point_id=pid), "BAD_ARG"), (dict(tile_off=off), "BAD_ARG"), (dict(tile_frame=tf), "BAD_ARG"), (dict(tile_cam=tcam), "BAD_ARG"),
                         (dict(lam=0.0), "BAD_ARG"), (dict(lam=float("nan")), "BAD_ARG"), (dict(lam=float("inf")), "BAD_ARG"), (dict(cameras=[(9, K, T, fl)]), "BAD_ARG"),
                         (dict(cameras=[(m, K, T, 8)]), "BAD_ARG"), (dict(cameras=[(m, [np.nan] + list(K[1:]), T, fl)]), "BAD_ARG"),
                         (dict(points=a["points"][:3], nominal=a["nominal"][:3], point_id=a["point_id"] % 3), "BAD_ARG"),
                         (dict(cameras=tc.unsupported_case()["cameras"]), "UNSUPPORTED")):
        msg = _rc(_call, case, 99, **change)
        assert code in msg, (list(change), msg)
    big = np.zeros((1025, 3)); big[:, 0] = np.arange(1025)
    assert "UNSUPPORTED" in _rc(_call, case, 99, points=big, nominal=big)
    L = lib.load()
    assert L.vc_target_refine_batch(0, 1, *([None] * 4), 1, None, 0, *([None] * 7), 21, C.c_double(1.0), *([None] * 8)) == -2          # null pointers
    assert "BAD_ARG" in _rc(lib.time_target_refine_batch, **tc.lib_args(case), device=99, reps=0)


def test_a_device_that_does_not_exist_is_no_device():
    assert "NO_DEVICE" in _rc(_call, tc.cases()["p21_n5"], 99)


@pytest.mark.skipif(_have_gpu(), reason="GPU present: the call would run")
def test_no_cpu_fallback_without_device():
    case = tc.cases()["p21_n5"]
    assert "NO_DEVICE" in _rc(_call, case, 0)
    assert "NO_DEVICE" in _rc(lib.time_target_refine_batch, **tc.lib_args(case), reps=2)


def test_cli_flag_errors(tmp_path):
    """the tool says what is wrong with the flags and exits with status 1 before it reads anything"""
    import os
    import subprocess
    BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vicalib_amd", "vicalib")
    for bad, word in ((["-refine_target_rounds", "-1"], "refine_target_rounds"),
                      (["-refine_target_rounds", "1", "-gpus", "2"], "gpus"),
                      (["-refine_target_rounds", "1", "-holdout_every", "5"], "holdout_every"),
                      (["-refine_target_rounds", "1", "-dot_bias_rounds", "1"], "dot_bias_rounds"),
                      (["-refine_target_rounds", "1", "-imu", "csv://imu"], "nocalibrate_imu"),
                      (["-refine_target_rounds", "1", "-refine_target_sigma", "0"], "refine_target_sigma"),
                      (["-refine_target_rounds", "1", "-refine_target_output", ""], "refine_target_output")):
        r = subprocess.run([BIN, "-cam", "detections://missing.txt"] + bad, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
        assert r.returncode == 1 and word in r.stderr, (bad, r.returncode, r.stderr[-300:])
    assert not os.path.exists(tmp_path / "target_refined.csv")
