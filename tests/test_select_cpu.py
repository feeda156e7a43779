"""Greedy D-optimal view selection (vc_selector*), the part that needs no GPU: the selection's arithmetic (vc_select.hpp) compiled for the host and
held to the numpy reference of tests/select_ref.py by the checks of tests/select_cases.py -- the same checks tests/test_select_gpu.py applies to the
kernels --, the properties of the definition, argument errors, the refusal to run without a device and the command line's flag errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import select_cases as sc
import select_ref as ref
import vicalib_amd.lib as lib
from vicalib_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")
NUMERIC_NAMES = [n for n in sc.NAMES if sc.cases()[n]["numeric"]]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


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
            rc, out = sc.host_select(sc.cases()[name])
            assert rc == 0
            cache[name] = out
        return cache[name]
    return get


@pytest.mark.parametrize("name", sc.NAMES)
def test_information_matches_analytic_reference(runs, name):
    sc.check_information(name, runs(name))


@pytest.mark.parametrize("name", NUMERIC_NAMES)
def test_information_and_gains_mean_what_the_definition_says(runs, name):
    """against central differences of the generator's projection: no closed form on the reference's side"""
    got, tol, a = runs(name), sc.numeric_tolerances(name), sc.analytic(name)
    err = float(np.abs(ref.scaled(got["I"], a["scale"]) - tol["It"]).max())
    rc, first = sc.host_select(sc.cases()[name], k=1)
    assert rc == 0
    eg = float(np.abs(first["last_gains"] - tol["gains"]).max())
    print(f"{name}: I_f against central differences {err:.3e} (tol {tol['I']:.3e}), first-round gains {eg:.3e} (tol {tol['gain']:.3e})")
    assert err <= tol["I"]
    assert eg <= tol["gain"]


@pytest.mark.parametrize("name", sc.NAMES)
def test_selection_follows_the_pick_rule(runs, name):
    got = runs(name)
    sc.check_selection(name, got)
    if sc.separation(name) >= sc.SEPARATION:          # well-separated gains: the sequence itself is pinned
        assert np.array_equal(got["order"], sc.selection(name, True)["order"])


def test_exact_sequence_cases_are_well_separated():
    """every case but the one with two identical frames has the reference's best and second-best gains >= 1000 tolerances apart in every round"""
    for n in sc.NAMES:
        assert (sc.separation(n) >= sc.SEPARATION) == (n != "poly3_67"), (n, sc.separation(n))


def test_unsupported_beyond_64_columns():
    rc, _ = sc.host_select(sc.unsupported_case())
    assert rc == -7


def test_gains_never_grow(runs):
    name = "stereo_fov"
    tol = sc.tolerances(name)["gain"]
    prev = None
    for k in (1, 2, 3):
        rc, out = sc.host_select(sc.cases()[name], k=k)
        assert rc == 0
        g = out["last_gains"]
        if prev is not None:
            left = g >= 0
            assert np.all(g[left] <= prev[left] + tol)
            assert (g < 0).sum() == (prev < 0).sum() + 1
        prev = g


def test_all_frames_selected_reach_total(runs):
    name = "k_equals_n"
    got, tol = runs(name), sc.tolerances(name)
    assert len(got["order"]) == 5
    assert abs(got["cum"][-1] - got["total"]) <= tol["cum"] + tol["total"]
    assert np.all(np.diff(got["cum"]) > 0) and np.all(np.diff(got["gain"]) <= tol["gain"])


def test_mixed_recording(runs):
    """the 3-corner frame is underdetermined and never picked, a corner behind the camera is counted and its frame stays usable, the second of two
    identical frames gains strictly less than the first did, k > usable ends when the candidates do"""
    name = "poly3_67"
    got, sp = runs(name), sc.cases()[name]["special"]
    assert got["status"][sp["three"]] == 1 and got["corners"][sp["three"]] == 3 and sp["three"] not in got["order"]
    assert got["status"][sp["behind"]] == 2 and got["behind"][sp["behind"]] == 1 and sp["behind"] in got["order"]
    assert len(got["order"]) == 66
    a, b = sp["twins"]
    assert np.array_equal(got["I"][a], got["I"][b])
    ka, kb = int(np.where(got["order"] == a)[0][0]), int(np.where(got["order"] == b)[0][0])
    assert ka < kb and got["gain"][kb] < got["gain"][ka]
    rc, first = sc.host_select(sc.cases()[name], k=1)
    assert rc == 0 and first["last_gains"][a] == first["last_gains"][b] and first["last_gains"][sp["three"]] == -1.0


def test_units_of_a_camera_do_not_matter(runs):
    """the image measured in thousandths of a pixel (fu, fv, cu, cv x 1000): every entry of I_f moves by a power of 1000, order and gains stay"""
    name = "mono_poly3"
    c = dict(sc.cases()[name])
    m, K, T, fl = c["cameras"][0]
    c["cameras"] = [(m, [k * 1000.0 for k in K[:4]] + list(K[4:]), T, fl)]
    rc, out = sc.host_select(c)
    assert rc == 0
    got, tol = runs(name), sc.tolerances(name)
    assert np.array_equal(out["order"], got["order"])
    assert np.abs(out["gain"] - got["gain"]).max() <= tol["gain"] and abs(out["total"] - got["total"]) <= tol["total"]
    assert out["I"][0][4, 4] == pytest.approx(1e6 * got["I"][0][4, 4], rel=1e-9) and out["I"][0][0, 0] == pytest.approx(got["I"][0][0, 0], rel=1e-9)


def test_scaling_does_not_change_a_gain():
    """purely numerical: differences of log-determinants do not depend on the column scaling.  The prior is stated on the scaled columns, so the claim
    is about the data term: with frame 0 as start set and a prior far below it (1e-30), the long-double reference gives the same gains from I_f as
    from diag(s) I_f diag(s), to 1e-12 of the largest"""
    a = sc.analytic("mono_poly3", True)
    g_s = ref.gains_given(a["It"], a["status"], ref.start_matrix(a["It"], (0,), 1e-30), {0})
    g_u = ref.gains_given(a["I"], a["status"], ref.start_matrix(a["I"], (0,), 1e-30), {0})
    assert g_s[0] == -1 and np.abs(g_s - g_u)[1:].max() <= 1e-12 * np.abs(g_s[1:]).max(), (g_s, g_u)


def test_start_set_is_a_continuation(runs):
    name = "stereo_fov"
    full = runs(name)
    f0 = int(full["order"][0])
    rc, cont = sc.host_select(sc.cases()[name], k=3, start=[f0])
    assert rc == 0
    tol = sc.tolerances(name)
    assert np.array_equal(cont["order"], full["order"][1:])
    assert np.abs(cont["gain"] - full["gain"][1:]).max() <= tol["gain"]
    assert np.abs(cont["cum"] - (full["cum"][1:] - full["cum"][0])).max() <= 2 * tol["cum"]


def test_threads_do_not_change_a_bit(runs):
    name = "stereo_fov"
    rc, out = sc.host_select(sc.cases()[name], threads=4)
    assert rc == 0
    got = runs(name)
    assert np.array_equal(out["order"], got["order"]) and np.array_equal(out["gain"], got["gain"]) and np.array_equal(out["I"], got["I"])


def test_claim_selected_views_beat_the_subsample():
    """60 frames, 50 near-duplicate fronto-parallel and 10 tilted and close: the reference's log-determinant of the 10 selected views exceeds that of
    the every-6th subsample.  Margin found: 43.5 (selected 84.4 against 40.9, of 86.3 attainable); the ten selected are exactly the ten tilted views."""
    name = "claim_poly3_60"
    a, c = sc.analytic(name, True), sc.cases()[name]
    sel = sc.selection(name, True)
    S0 = ref.start_matrix(a["It"], (), c["prior"])
    every6 = list(range(0, 60, 6))
    ld_sel = float(ref.logdet(S0 + sum(a["It"][f] for f in sel["order"])) - ref.logdet(S0))
    ld_sub = float(ref.logdet(S0 + sum(a["It"][f] for f in every6)) - ref.logdet(S0))
    print(f"selected {ld_sel:.3f}, every 6th {ld_sub:.3f}, total {float(sel['total']):.3f}, picks {sel['order']}")
    assert len(sel["order"]) == 10 and ld_sel > ld_sub + 20.0
    rc, got = sc.host_select(c)
    assert rc == 0 and np.array_equal(got["order"], sel["order"])
    assert set(got["order"].tolist()) == set(range(3, 60, 6))


# ---------------------------------------------------------------------------------------------- the C ABI without a device
def _create(cameras, device=0):
    L = lib.load()
    model, params, T_ck, flags = sc.rig_arrays(cameras)
    nparams = np.array([len(c[1]) for c in cameras], dtype=np.int32)
    h = C.c_void_p()
    rc = L.vc_selector_create(int(device), len(cameras), _p(model), _p(params), _p(nparams), _p(T_ck), _p(flags), C.byref(h))
    return rc, h


def test_create_argument_errors_come_before_the_device():
    L = lib.load()
    cams = sc.cases()["mono_poly3"]["cameras"]
    m, K, T, fl = cams[0]
    assert _create([(m, K[:-1], T, fl)])[0] == -2                    # nparams does not fit the model
    assert _create([(m, K, T, 8)])[0] == -2                          # an unknown flag
    assert _create([(m, K, T, 0)])[0] == -2                          # nothing free: D = 0
    assert _create([(m, [np.nan] + list(K[1:]), T, fl)])[0] == -2
    assert _create(sc.unsupported_case()["cameras"])[0] == -7        # D = 74 > 64: VC_ERR_UNSUPPORTED
    assert _create(sc.rig("poly3", 2) * 5)[0] == -2                  # more than 8 cameras
    h = C.c_void_p()
    assert L.vc_selector_create(0, 0, None, None, None, None, None, C.byref(h)) == -2
    for reader in ("vc_select_dim",):
        assert getattr(L, reader)(None) == -2
    assert L.vc_select_run(None, 1, None, 0, C.c_double(1e-6)) == -2


def test_no_cpu_fallback_without_device():
    if _have_gpu():
        pytest.skip("GPU present")
    rc, h = _create(sc.cases()["mono_poly3"]["cameras"])
    assert rc == -1 and not h.value                                  # VC_ERR_NO_DEVICE
    with pytest.raises(lib.VicalibError):
        lib.Selector(sc.cases()["mono_poly3"]["cameras"])


def _cli(*args):
    return subprocess.run([BIN] + list(args), capture_output=True, text=True, timeout=60)


def test_cli_flag_errors(tmp_path):
    """-select_views without -select_dir, K < 1, a parent directory that does not exist, a prior that is not > 0, a start set that is no list of frames:
    the tool says so and exits with status 1 before it reads anything"""
    out = str(tmp_path / "o")
    for bad, word in ((["-select_views", "5"], "select_dir"),
                      (["-select_views", "0", "-select_dir", out], "select_views"),
                      (["-select_views", "x", "-select_dir", out], "select_views"),
                      (["-select_dir", out], "select_views"),
                      (["-select_views", "5", "-select_dir", str(tmp_path / "no" / "such" / "o")], "does not exist"),
                      (["-select_views", "5", "-select_dir", out, "-select_prior", "0"], "select_prior"),
                      (["-select_views", "5", "-select_dir", out, "-select_start", "1,x"], "select_start"),
                      (["-select_views", "5", "-select_dir", out, "-gpus", "2"], "gpus")):
        r = _cli("-cam", "detections://missing.txt", *bad)
        assert r.returncode == 1 and word in r.stderr, (bad, r.returncode, r.stderr[-300:])
    assert not os.path.exists(out)
