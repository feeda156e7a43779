"""The depth calibration (vc_depthcal*), the part that needs no GPU: the command line's flags and argument errors, the refusal to run
without a device, argument checks that come before the device, the conditions the cases must meet (from the reference alone), and the
kernels' arithmetic (vc_depthcal.hpp) compiled for the host and held to the same checks against the numpy reference that
tests/test_depthcal_gpu.py applies to the kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import depthcal_cases as dc
import depthcal_ref as dr
import register_cases as rc
import vicalib_amd.lib as lib
from vicalib_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(HERE), "vicalib_amd", "vicalib")
FLAGS = ("-depthcal_models", "-depthcal_cam", "-depthcal_poses", "-depthcal_depth", "-depthcal_dir", "-depthcal_apply", "-depthcal_interp", "-depthcal_unit",
         "-depthcal_kind", "-depthcal_bins", "-depthcal_vref", "-depthcal_min_cos", "-depthcal_max_dev", "-depthcal_degree", "-depthcal_min_count",
         "-depthcal_min_spread", "-depthcal_margin")


def _have_gpu():
    n = C.c_int(0)
    return lib.hip_runtime().hipGetDeviceCount(C.byref(n)) == 0 and n.value > 0


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _run(*args):
    return subprocess.run([BIN] + list(args), capture_output=True, text=True, timeout=60)


def _inputs(tmp_path, n=2):
    return dc.tool_inputs(tmp_path, dc.tool_case("main"), n)


def _replace(args, flag, value):
    args = list(args)
    args[args.index(flag) + 1] = value
    return args


# ------------------------------------------------------------------------------------------------------------ the tool
def test_cli_lists_the_depthcal_flags():
    r = _run("-help")
    assert r.returncode == 0
    for flag in FLAGS:
        assert flag + " " in r.stdout, flag
    r = _run("-depthcal_models", "/does/not/exist.xml", "-depthcal_poses", "/none.csv", "-depthcal_depth", "file:///does/not/exist_*.pgm", "-depthcal_dir", "out")
    assert r.returncode == 1 and "cannot open rig file" in r.stderr and "unknown command line flag" not in r.stderr


@pytest.mark.parametrize("flag, value, message", [
    ("-depthcal_kind", "depth", "depthcal_kind"), ("-depthcal_unit", "0", "depthcal_unit"), ("-depthcal_bins", "4", "depthcal_bins"), ("-depthcal_bins", "33,3", "depthcal_bins"),
    ("-depthcal_vref", "0", "depthcal_vref"), ("-depthcal_min_cos", "1.5", "depthcal_min_cos"), ("-depthcal_max_dev", "-1", "depthcal_max_dev"),
    ("-depthcal_degree", "3", "depthcal_degree"), ("-depthcal_min_count", "0", "depthcal_min_count"), ("-depthcal_min_spread", "-1", "depthcal_min_spread"),
    ("-depthcal_margin", "-2", "depthcal_margin"), ("-depthcal_cam", "1", "depthcal_cam"), ("-depthcal_cam", "-1", "depthcal_cam")])
def test_cli_argument_errors(tmp_path, flag, value, message):
    r = _run(*_replace(_inputs(tmp_path), flag, value))
    assert r.returncode == 1 and message in r.stderr, r.stderr
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("extra, message", [
    (["-compare_models", "a.xml,b.xml", "-compare_dir", "cmp"], "exclude each other"), (["-convert_models", "a.xml", "-convert_to", "kb4"], "exclude each other"),
    (["-register_models", "a.xml", "-register_depth", "file://x_*.pgm", "-register_dir", "reg"], "exclude each other"),
    (["-depthcal_apply", "depth_correction.csv"], "exclude each other"), (["-depthcal_interp", "cubic"], "depthcal_interp")])
def test_cli_exclusions(tmp_path, extra, message):
    r = _run(*(_inputs(tmp_path) + extra))
    assert r.returncode == 1 and message in r.stderr, r.stderr
    assert not (tmp_path / "out").exists()


def test_cli_needs_depth_dir_and_poses(tmp_path):
    args = _inputs(tmp_path)
    r = _run(*args[:6])
    assert r.returncode == 1 and "-depthcal_dir" in r.stderr
    r = _run(*(args[:4] + args[6:]))                         # without -depthcal_poses
    assert r.returncode == 1 and "-depthcal_poses" in r.stderr
    assert not (tmp_path / "out").exists()


def test_cli_mismatched_counts_name_both_numbers(tmp_path):
    args = _inputs(tmp_path, n=3)
    os.remove(tmp_path / "depth_02.pgm")
    r = _run(*args)
    assert r.returncode == 1 and "2 files" in r.stderr and "3 frames" in r.stderr, r.stderr
    assert not (tmp_path / "out").exists()


def test_cli_refuses_large_headers_and_wrong_sizes(tmp_path):
    args = _inputs(tmp_path, n=2)
    with open(tmp_path / "depth_00.pgm", "wb") as f:
        f.write(b"P5\n2000000 2000000\n65535\n\0\0")
    r = _run(*args)
    assert r.returncode == 1 and "8192 x 8192" in r.stderr, r.stderr
    rc.write_pgm16(tmp_path / "depth_00.pgm", np.zeros((9, 9), dtype=np.uint16))
    r = _run(*args)
    assert r.returncode == 1 and "9 x 9 pixels" in r.stderr, r.stderr
    with open(tmp_path / "poses.csv", "a") as f:
        f.write("1 2 3\n")
    r = _run(*args)
    assert r.returncode == 1 and "12 numbers" in r.stderr, r.stderr
    assert not (tmp_path / "out").exists()


def test_cli_apply_refuses_a_bad_correction_file(tmp_path):
    args = _inputs(tmp_path, n=1)
    with open(tmp_path / "corr.csv", "w") as f:
        f.write("size,67,35\nbins,4,3\nv_ref,1000\n")
    r = _run("-depthcal_apply", str(tmp_path / "corr.csv"), "-depthcal_depth", args[7], "-depthcal_dir", str(tmp_path / "out"))
    assert r.returncode == 1 and "not a depth correction file" in r.stderr, r.stderr
    assert not (tmp_path / "out").exists()


def test_cli_without_device(tmp_path):
    if _have_gpu():
        pytest.skip("GPU present")
    r = _run(*_inputs(tmp_path))
    assert r.returncode == 3 and "no HIP device" in r.stderr


# ------------------------------------------------------------------------------------------------------------ the library's checks
def _create(L, **kw):
    s = dc.case("main")["setup"]
    a = dict(model=synth.MODEL_IDS[s.cam[0]], K=s.cam[1], nk=len(s.cam[1]), w=s.size[0], h=s.size[1], T=s.cam[3], unit=s.unit, kind=s.kind, rect=s.rect, bx=4, by=3,
             v_ref=s.v_ref, min_cos=s.min_cos, max_dev=s.max_dev)
    a.update(kw)
    h = C.c_void_p()
    d = lambda x: None if x is None else _p(np.ascontiguousarray(x, dtype=np.float64))      # noqa: E731
    st = L.vc_depthcal_create(0, a["model"], d(a["K"]), a["nk"], a["w"], a["h"], d(a["T"]), C.c_double(a["unit"]), a["kind"], d(a["rect"]), a["bx"], a["by"],
                              C.c_double(a["v_ref"]), C.c_double(a["min_cos"]), C.c_double(a["max_dev"]), C.byref(h))
    return st, h


def test_no_cpu_fallback_without_device():
    if _have_gpu():
        pytest.skip("GPU present")
    L = lib.load()
    status, h = _create(L)
    assert status == -1 and not h.value                      # VC_ERR_NO_DEVICE
    with pytest.raises(lib.VicalibError):
        lib.DepthCalibrator(**dc.setup_args(dc.case("main")["setup"]))


def test_arguments_are_checked_before_the_device():
    L = lib.load()
    long_q = rc.T_S.copy(); long_q[:4] *= 1.0 + 1e-5
    bad = [dict(model=9), dict(nk=6), dict(w=1), dict(h=8193), dict(T=long_q), dict(T=None), dict(K=None), dict(unit=0.0), dict(unit=np.inf), dict(kind=2), dict(kind=-1),
           dict(rect=None), dict(rect=(0.5, 0, 0.5, 1)), dict(rect=(0, 1, 1, 0)), dict(rect=(0, 0, np.nan, 1)), dict(bx=0), dict(bx=33), dict(by=0), dict(by=33),
           dict(v_ref=0.0), dict(v_ref=np.nan), dict(min_cos=0.0), dict(min_cos=1.01), dict(max_dev=0.0), dict(max_dev=np.inf)]
    for kw in bad:
        status, h = _create(L, **kw)
        assert status == -2 and not h.value, kw              # VC_ERR_BAD_ARG, also where there is no device
    buf = np.zeros(64)
    ll = C.c_longlong
    assert L.vc_depthcal_add(None, 1, _p(buf), 4, ll(4), _p(buf), None) == -2
    assert L.vc_depthcal_expected(None, 1, _p(buf), None, 0, ll(0), _p(buf), _p(buf)) == -2
    assert L.vc_depthcal_sums(None, None, None, None, None) == -2 and L.vc_depthcal_clear(None) == -2
    assert L.vc_depthcal_fit(None, 2, 50, C.c_double(0.02)) == -2 and L.vc_depthcal_get_fit(None, None, None, None, None, None, None) == -2
    assert L.vc_depthcal_set_fit(None, 2, _p(buf), _p(buf), _p(buf)) == -2
    assert L.vc_depthcal_apply(None, 1, _p(buf), 4, ll(4), _p(buf), 4, ll(4), 0, None) == -2
    assert L.vc_depthcal_get(None, None, None, None, None, None, None, None, None, None, None) == -2
    assert L.vc_time_depthcal(None, 1, 1, _p(buf)) == -2
    assert L.vc_depthcal_create_for_camera(None, 0, C.c_double(0.001), 0, _p(buf), 4, 3, C.c_double(1000), C.c_double(0.5), C.c_double(100), C.byref(C.c_void_p())) == -2


# ------------------------------------------------------------------------------------------------------------ the cases, from the reference alone
@pytest.mark.parametrize("name", dc.CASES)
def test_cases_are_decided(name):
    c = dc.case(name)
    dc.assert_decided(c)
    assert np.all(c["acc"]["counters"].sum(axis=1) == c["setup"].size[0] * c["setup"].size[1])
    assert c["acc"]["counters"][dc.NOTHING][7] == 0          # a frame that contributes nothing


def test_cases_meet_the_conditions():
    total = sum(dc.case(name)["acc"]["counters"].sum(axis=0) for name in dc.CASES)
    assert np.all(total > 0), total                          # every rule is met by some case
    assert dc.case("beyond")["acc"]["counters"][:, 1].sum() > 0 and dc.case("small_unit")["acc"]["counters"][:, 5].sum() > 0
    main = dc.case("main")
    assert np.all(main["acc"]["sums"][:, 0] >= dc.MIN_COUNT)                      # every cell of the main case is populated
    assert np.all(main["acc"]["counters"].sum(axis=0)[[0, 2, 3, 4, 6, 7]] > 0)
    seen = set(int(s) for s in dr.fit(dc.case("range")["acc"]["sums"], 2, dc.MIN_COUNT, dc.MIN_SPREAD)["status"])
    assert seen == {0, 1, 2}                                 # all three statuses
    fine = dc.case("fine")["setup"]
    heights = np.bincount(fine.cell_map()[:, 0] // 32)
    assert set(heights[heights > 0]) == {1, 2}               # cells one or two pixels high
    assert dc.BIG[0] * dc.BIG[1] > 4 * 1024                  # a cell longer than any one chunk, also when the image is cut in two


def test_reference_fit_recovers_what_was_planted():
    c = dc.case("main")
    f = dr.fit(c["acc"]["sums"], 2, dc.MIN_COUNT, dc.MIN_SPREAD)
    assert f["rms"][0] > 4.0 and f["rms"][1] < 0.5 * f["rms"][0] and f["rms"][2] < 0.5        # the rounding of the values alone is 0.29
    assert dr.fit(np.zeros((12, 9)), 2, 1, 0.0) is None


# ------------------------------------------------------------------------------------------------------------ the host build against the reference
def test_host_expected_against_the_reference():
    worst = 0.0
    for name in dc.CASES:
        c = dc.case(name)
        worst = max(worst, dc.check_expected(dc.make_host(c["setup"]), c))
    print("deviation of the host build in y: %.3g counts" % worst)
    assert worst <= dc.D_Y, worst


@pytest.mark.parametrize("name", dc.SUM_CASES)
def test_host_sums_against_the_reference(name):
    c = dc.case(name)
    ratio = dc.check_sums(dc.make_host(c["setup"]), c)
    print("largest deviation of a sum over its bound: %.3g" % ratio)


@pytest.mark.parametrize("name", ["main", "big_two"])
def test_host_reproducible(name):
    dc.check_reproducible(dc.make_host, dc.case(name))


def test_host_fit_against_the_reference():
    worst, seen = 0.0, set()
    for name in dc.SUM_CASES:
        c = dc.case(name)
        w, s = dc.check_fit(dc.make_host(c["setup"]), c)
        worst = max(worst, w); seen |= s
    print("deviation of the host fit from the numpy fit on identical sums: %.3g counts" % worst)
    assert worst <= dc.D_FIT and seen == {0, 1, 2}, (worst, seen)


def test_host_fit_refuses_what_cannot_be_fitted():
    assert dc.fit_sums_host(np.zeros((12, 9)), 2, 1, 0.0) is None
    one = np.zeros((1, 9)); one[0] = [5, 0, 0, 0, 0, 10, 0, 0, 20]               # five pixels of one value: no slope
    assert dc.fit_sums_host(one, 1, 1, 0.0) is None and dc.fit_sums_host(one, 0, 1, 0.0)["c"][0] == 2.0
    h = dc.make_host(dc.case("main")["setup"])
    with pytest.raises(LookupError):
        h.get_fit()                                          # no fit yet
    dc.add_all(h, dc.case("main")); h.fit(2, dc.MIN_COUNT, dc.MIN_SPREAD); h.get_fit()
    h.add(dc.case("main")["depth"][:1], dc.case("main")["poses"][:1])
    with pytest.raises(LookupError):
        h.get_fit()                                          # stale


@pytest.mark.parametrize("name", ["main", "range"])
def test_host_apply_against_the_reference(name):
    excluded = dc.check_apply(dc.make_host, dc.case(name))
    print("pixels excluded as undecided: %d" % excluded)


def test_host_end_to_end():
    before, after, after_ref = dc.check_end_to_end(dc.make_host, dc.case("main"))
    print("raw rms on held-out frames: %.3g counts before, %.3g after (reference %.3g)" % (before, after, after_ref))
