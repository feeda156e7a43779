"""The odd-even elimination of the chain's upper levels (k_chain_oe, the top level in k_chain_top_gram, chain_back_oe) against the
dense reference step of tests/lm_step_ref.py -- test_lm_step_gpu's check_case and its bounds, nothing of its own.  Mono kb4, D = 29.
Frame counts are the smallest at which each branch of the schedule can go wrong: a last level-1 group with q = 1 .. 7 interior separators
behind a full group that has a right separator, a single full group without one, a top level of 1 .. 7 frames, and two odd-even levels.
The switch (VICALIB_AMD_CHAIN_ODD_EVEN) is read when a calibrator is created: a case sets its environment first and runs in-process.
A whole 130-frame calibration with the switch on and off must agree the way test_fold_gpu's two forms do."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import test_lm_step_gpu as lm      # noqa: E402

pytestmark = pytest.mark.gpu
SWITCHES = ("VICALIB_AMD_CHAIN_ODD_EVEN", "VICALIB_AMD_BACK_PATH", "VICALIB_AMD_FOLD_L0")

# level 1: last group with q interior separators (73 .. 121), an exact fit (128), one full group without a right separator (57)
LEVEL1 = [73, 81, 89, 97, 105, 113, 121, 128, 57]
# top level with t = 2 .. 7 frames
TOP = [100, 130, 200, 260, 330, 448]
# two odd-even levels: level 2 = one full group with a right separator + a group with q = 2
TWO_LEVELS = [648]


def _levels(n_frames):
    """levels below the top one (vc_chain_plan.hpp: strides 1, 8, 64, .. while more than 7 frames are active)"""
    n, st = 0, 1
    while (n_frames - 1) // st + 1 > 7:
        n += 1
        st *= 8
    return n


def _check(monkeypatch, n_frames, odd_even=True, paths=None, **env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if not odd_even:
        monkeypatch.setenv("VICALIB_AMD_CHAIN_ODD_EVEN", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    # the report of the calibrator check_case itself builds: taken where it asks for the forms of the pass
    seen = {}
    paths_of = lm.ViCalibrator.pass_paths

    def pass_paths(self):
        seen["order"] = self.chain_order()
        return paths_of(self)

    monkeypatch.setattr(lm.ViCalibrator, "pass_paths", pass_paths)
    lm.check_case(lm._i(("kb4",), n_frames, 29, paths=paths))
    order = seen["order"]
    print("chain order", order)
    nl = _levels(n_frames)
    assert order["n_levels"] == nl
    assert order["oe"] == [1 if (odd_even and l >= 1) else 0 for l in range(nl)]
    assert order["oe_top"] == (1 if odd_even else 0)


@pytest.mark.parametrize("n_frames", LEVEL1 + TOP + TWO_LEVELS)
def test_odd_even_step_matches_dense_reference_solve(monkeypatch, n_frames):
    _check(monkeypatch, n_frames, paths=lm.ON)


@pytest.mark.parametrize("n_frames", [130, 648])
def test_switch_off_keeps_the_two_sided_levels(monkeypatch, n_frames):
    _check(monkeypatch, n_frames, odd_even=False, paths=lm.ON)


def test_odd_even_with_the_level_by_level_back_substitution(monkeypatch):
    _check(monkeypatch, 130, paths=dict(back_path=0), VICALIB_AMD_BACK_PATH=0)


def test_odd_even_without_the_folded_bottom_level(monkeypatch):
    _check(monkeypatch, 130, paths=dict(fold_l0=0), VICALIB_AMD_FOLD_L0=0)


def _run(tmp_path, name, n_frames, **env):
    out = str(tmp_path / (name + ".npz"))
    e = dict(os.environ)
    for k in SWITCHES:
        e.pop(k, None)
    e.update({k: str(v) for k, v in env.items()})
    r = subprocess.run([sys.executable, os.path.join(HERE, "sync_worker.py"), out, str(n_frames)], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)


def test_whole_calibration_agrees_with_the_switch_off(tmp_path):
    a = _run(tmp_path, "oe", 130, VICALIB_AMD_CHAIN_ODD_EVEN=1)
    b = _run(tmp_path, "two", 130, VICALIB_AMD_CHAIN_ODD_EVEN=0)
    assert int(a["timeouts"]) == 0 and int(b["timeouts"]) == 0
    ta, tb = a["trace"], b["trace"]
    assert ta.shape == tb.shape and len(ta) > 20
    np.testing.assert_array_equal(ta[:, 8], tb[:, 8])                     # accept / reject
    print("cost: max relative difference %.3e" % np.max(np.abs(ta[:, 1] - tb[:, 1]) / np.abs(tb[:, 1])))
    print("intrinsics: max relative difference %.3e" % np.max(np.abs(a["K"] - b["K"]) / np.abs(b["K"])))
    np.testing.assert_allclose(ta[:, 1], tb[:, 1], rtol=1e-7)             # cost of every iteration
    np.testing.assert_allclose(a["K"], b["K"], rtol=1e-8)
    np.testing.assert_allclose(a["frames"], b["frames"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(a["biases"], b["biases"], rtol=1e-7, atol=1e-11)
    assert abs(float(a["toff"]) - float(b["toff"])) < 1e-11
