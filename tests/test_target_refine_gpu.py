"""The target step on the device (vc_target_refine_batch: sweep, assembly, elimination of the shared columns, gauge, blocked Cholesky, solve) against
the numpy reference of tests/target_refine_ref.py, by the checks of tests/target_refine_cases.py -- the same the host build meets in
tests/test_target_refine_cpu.py --, the bits (a second run, a second call, an empty frame appended), the properties and the argument errors."""
import ctypes as C

import numpy as np
import pytest

import target_refine_cases as tc
import vicalib_amd.lib as lib

pytestmark = pytest.mark.gpu


def _run(case, **kw):
    return lib.target_refine_batch(**tc.lib_args(case), out=dict(refined=np.full((len(case["points"]), 3), tc.FILL)), **kw)


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run(tc.cases()[name])
        return cache[name]
    return get


@pytest.mark.parametrize("name", tc.NAMES)
def test_step_matches_reference(runs, name):
    tc.check(name, runs(name), " (device)")


def test_host_build_and_device_agree(runs):
    """the same arithmetic in another order: within the sum of their bounds"""
    for name in ("stereo_fov", "p117_views"):
        rc, host = tc.host_step(tc.cases()[name])
        assert rc == 0
        assert np.abs(host["refined"] - runs(name)["refined"]).max() <= 2 * tc.bounds(name)[0]["refined"]
        assert np.array_equal(host["point_corners"], runs(name)["point_corners"])


def _same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("refined", "point_status", "point_corners", "cost", "predicted_decrease", "gauge_rank"))


@pytest.mark.parametrize("name", ["stereo_fov", "p117_views", "p21_n67"])
def test_same_bits(runs, name):
    """a second run; a second call after another case has used the device; the frames with an empty one appended"""
    case = tc.cases()[name]
    first = runs(name)
    assert _same(first, _run(case))
    _run(tc.cases()["mono_kb4"])
    assert _same(first, _run(case))
    more = dict(case); more["poses"] = np.concatenate([case["poses"], case["poses"][:1]])
    got = _run(more)
    assert _same(first, got)
    assert got["frame_status"][-1] == 1 and got["corners"][-1] == 0 and np.array_equal(got["frame_status"][:-1], first["frame_status"])


def test_exact_measurements_give_no_step(runs):
    got, case = runs("exact"), tc.cases()["exact"]
    assert np.abs(got["refined"] - case["nominal"]).max() <= tc.bounds("exact")[0]["refined"]


def test_similarity_in_points_changes_nothing(runs):
    """on the exact case (tests/test_target_refine_cases_cpu.py says why there)"""
    moved = _run(tc.moved_by_small_similarity("exact"))
    assert np.abs(moved["refined"] - runs("exact")["refined"]).max() <= tc.bounds("exact")[0]["refined"]


def test_similarity_in_points_with_a_real_step(runs):
    """a noisy case, d != 0: `refined` moves by no more than the step turns with the board (tc.similarity_bound), some 50 times less than the similarity"""
    name = "mono_poly3"
    moved = _run(tc.moved_by_small_similarity("mono_poly3"))
    shift = np.abs(moved["refined"] - runs(name)["refined"]).max()
    delta = np.abs(tc.moved_by_small_similarity(name)["points"] - tc.cases()[name]["points"]).max()
    print("similarity %.3e m moves refined by %.3e m, bound %.3e m" % (delta, shift, tc.similarity_bound(name)))
    assert delta >= 20.0 * tc.similarity_bound(name)
    assert shift <= tc.similarity_bound(name)


def test_unobserved_rows_keep_their_bits(runs):
    got, case = runs("mixed"), tc.cases()["mixed"]
    sp = case["special"]
    for p in (sp["never"], sp["behind"]):
        assert got["point_status"][p] == 1 and got["point_corners"][p] == 0
        assert got["refined"][p].tobytes() == np.asarray(case["points"][p], dtype=np.float64).tobytes()
    assert got["point_corners"][sp["one_view"]] == 1 and got["behind"][sp["behind_frame"]] == 1 and got["frame_status"][sp["behind_frame"]] == 2


def test_argument_errors_and_unsupported():
    case = tc.cases()["p21_n5"]
    a = tc.lib_args(case)
    pid = a["point_id"].copy(); pid[0] = -1
    for change, code in ((dict(point_id=pid), "BAD_ARG"), (dict(lam=-1.0), "BAD_ARG"), (dict(cameras=tc.unsupported_case()["cameras"]), "UNSUPPORTED"),
                         (dict(points=a["points"][:3], nominal=a["nominal"][:3], point_id=a["point_id"] % 3), "BAD_ARG")):
        b = dict(a); b.update(change)
        with pytest.raises(lib.VicalibError, match=code):
            lib.target_refine_batch(**b)
    with pytest.raises(lib.VicalibError, match="NO_DEVICE"):
        lib.target_refine_batch(device=99, **a)


def test_stage_times_are_reported():
    ms = lib.time_target_refine_batch(**tc.lib_args(tc.cases()["stereo_fov"]), reps=2)
    assert list(ms) == list(lib.TARGET_REFINE_STAGES) and all(v > 0.0 for v in ms.values()), ms
