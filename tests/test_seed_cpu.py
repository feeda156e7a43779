"""The batched planar PnP (vc_pnp_planar_batch), the part that needs no GPU: its arithmetic (vc_seed.hpp) compiled for the host and run one view
at a time (tests/host_harness/seed_harness.cpp), held to the host routine it restates -- pnp_planar / pnp_planar_ransac -- by the checks of
tests/seed_cases.py, the same checks tests/test_seed_gpu.py applies to the kernel; the pick sequence against the contract's statement of it;
the entry point's argument errors and its refusal to run without a device; the command line's flag."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import seed_cases as sc
import vicalib_amd.lib as lib
from vicalib_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")
BAD_ARG, NO_DEVICE = -2, -1


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
            cache[name] = sc.host_seed(name)
        return cache[name]
    return get


def test_the_cases_cover_what_they_claim(runs):
    plain, robust = sc.group("plain")["views"], sc.group("robust")["views"]
    assert len(runs("plain")["status"]) == len(plain) and len(runs("robust")["status"]) == len(robust)      # (every view reaches the host build)
    assert [len(v["pw"]) for v in plain[:7]] == sc.COUNTS and [len(v["pw"]) for v in robust] == sc.ROBUST_COUNTS
    assert {v["model"] for v in plain} == set(sc.MODELS) and {v["model"] for v in robust} == set(sc.MODELS)
    assert any(v["pw"][0, 2] != 0.0 for v in plain) and any(v["pw"][0, 2] != 0.0 for v in robust)
    assert [v["expect"] for v in plain[-2:]] == [sc.FEW, sc.NOT_PLANAR] and sc.group("noise")["views"][0]["expect"] == sc.NO_CONSENSUS
    for v in robust:
        n = len(v["pw"])
        assert v["changed"].sum() == (max(1, n // 5) if n >= 8 else 0)
    assert [sc.group(g)["its"] for g in ("plain", "its1", "its64", "its65", "robust")] == [0, 1, 64, 65, 100]


@pytest.mark.parametrize("name", sc.GROUPS)
def test_host_build_matches_the_host_routine(runs, name):
    sc.check_against_host(name, runs(name), label=" (host build)")


def test_robust_views_flag_exactly_the_mismatched_corners(runs):
    got = runs("robust")
    for v, flags in zip(sc.group("robust")["views"], got["inlier"]):
        assert np.array_equal(~flags, v["changed"]), v["name"]


def test_refusals_and_untouched_outputs(runs):
    plain, noise = runs("plain"), runs("noise")
    assert plain["status"][-2:].tolist() == [sc.FEW, sc.NOT_PLANAR] and noise["status"].tolist() == [sc.NO_CONSENSUS, sc.OK]
    for got, k in ((plain, -2), (plain, -1), (noise, 0)):
        assert np.all(got["T_cw"][k] == -7.0) and got["rms"][k] == -7.0 and got["n_inliers"][k] == -7 and not got["inlier"][k].any()


def test_zero_iterations_and_fewer_than_five_corners_are_the_plain_branch():
    """its <= 0 || n < 5: all corners, one DLT, one refinement -- whatever the iteration count and the tolerance say"""
    H = sc.harness()
    v = sc.group("plain")["views"][0]
    assert len(v["pw"]) == 4
    K = np.zeros(10); K[:len(v["K"])] = v["K"]
    out = []
    for its, tol in ((0, 0.0), (100, 1e-9)):
        T = np.zeros(7); rms = C.c_double(0); n_in = C.c_int(0); flags = np.zeros(4, dtype=np.int8)
        assert H.seed_harness_view(synth.MODEL_IDS[v["model"]], sc._p(K), 4, sc._p(v["pw"]), sc._p(v["uv"]), its, C.c_double(tol), sc._p(T), C.byref(rms),
                                   C.byref(n_in), sc._p(flags)) == 0
        assert n_in.value == 4 and flags.all()
        out.append((T, rms.value))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]


@pytest.mark.parametrize("n", [5, 8, 190])
def test_pick_table_is_the_host_samplers(n):
    """index for index over 100 iterations: splitmix64 from 0x9E3779B97F4A7C15 ^ n, next() % n, a repeated pick redrawn, the draws running on
    through the iterations (pnp_planar_ransac keeps its sampler to itself; the identical inlier masks of the robust groups are its witness)"""
    table = sc.host_picks(n, 100)
    assert np.array_equal(table, sc.contract_picks(n, 100))
    assert all(len(set(row)) == 4 for row in table.tolist()) and table.min() >= 0 and table.max() < n


def _batch(n_views=2, model=None, K=None, off=None, pw=True, pc=True, its=0, tol=0.0, T=True, rms=True, n_in=True, status=True, inlier=True, device=0):
    L = lib.load()
    v = sc.group("plain")["views"][2]
    n = len(v["pw"])
    a = dict(model=np.array([synth.MODEL_IDS[v["model"]]] * 2, dtype=np.int32) if model is None else np.asarray(model, dtype=np.int32),
             K=np.zeros((2, 10)), off=np.array([0, n, 2 * n] if off is None else off, dtype=np.int32), pw=np.concatenate([v["pw"]] * 2),
             pc=np.concatenate([v["uv"]] * 2), T=np.zeros((2, 7)), rms=np.zeros(2), n_in=np.zeros(2, dtype=np.int32), status=np.zeros(2, dtype=np.int32),
             inlier=np.zeros(2 * n, dtype=np.int8))
    a["K"][:, :len(v["K"])] = v["K"]
    use = dict(model=model is not False, K=K is not False, off=off is not False, pw=pw, pc=pc, T=T, rms=rms, n_in=n_in, status=status, inlier=inlier)
    p = {k: (sc._p(a[k]) if use[k] else None) for k in a}
    return L.vc_pnp_planar_batch(device, n_views, p["model"], p["K"], p["off"], p["pw"], p["pc"], its, C.c_double(tol), p["T"], p["rms"], p["n_in"], p["inlier"],
                                 p["status"])


def test_argument_errors_come_before_the_device():
    for missing in ("model", "K", "off"):
        assert _batch(**{missing: False}) == BAD_ARG, missing
    for missing in ("pw", "pc", "T", "rms", "n_in", "status"):
        assert _batch(**{missing: False}) == BAD_ARG, missing
    assert _batch(n_views=-1) == BAD_ARG
    assert _batch(off=[0, 8, 7]) == BAD_ARG and _batch(off=[-1, 8, 16]) == BAD_ARG           # offsets that decrease; a negative start
    assert _batch(model=[2, 6]) == BAD_ARG and _batch(model=[-1, 2]) == BAD_ARG                # an unknown model
    assert _batch(its=-1) == BAD_ARG
    assert _batch(its=10, tol=-0.5) == BAD_ARG and _batch(its=10, tol=float("nan")) == BAD_ARG
    assert _batch(device=-1, its=-1) == BAD_ARG                                                # (the arguments are judged before the device)
    if not _have_gpu():          # no CPU fallback: a valid call without a device is refused, the optional flags missing or not
        assert _batch() == NO_DEVICE and _batch(inlier=False) == NO_DEVICE and _batch(n_views=0) == NO_DEVICE
        v = sc.group("plain")["views"][2]
        with pytest.raises(lib.VicalibError):
            lib.pnp_planar_batch([v["model"]], [v["K"]], [0, len(v["pw"])], v["pw"], v["uv"])


def test_help_lists_pnp_device():
    r = subprocess.run([BIN, "-help"], capture_output=True, text=True, timeout=60)
    assert "-pnp_device" in r.stdout + r.stderr
