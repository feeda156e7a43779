"""Converting a calibrated camera to another camera model (vc_convert*), the part that needs no GPU: the conversion's arithmetic and its
Levenberg-Marquardt driver (vc_convert.hpp) compiled for the host and held to the same numpy reference and the same checks that
tests/test_convert_gpu.py applies to the kernels, argument errors, the refusal to run without a device, and the command line's flag errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import compare_cases as cc
import convert_cases as cv
import rectify_cases as rc
import undistort_cases as uc
import vicalib_amd.lib as lib
from vicalib_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _harness():
    src = os.path.join(HERE, "host_harness", "convert_harness.cpp")
    so = os.path.join(HERE, "host_harness", "libvc_convert_harness.so")
    deps = [src] + [os.path.join(ROOT, "vicalib_amd", "csrc", f) for f in ("vc_convert.hpp", "vc_lm_rules.hpp", "vc_compare.hpp", "vc_rectify.hpp", "vc_undistort.hpp",
                                                                          "vc_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_convert(a, mb, fit_radius=1.0, max_iters=0, start=None, free_mask=0, size=cv.SIZE, grid=cv.GRID):
    """the host build of a whole conversion; (status, dict in the layout the checks take)"""
    ma, Ka = a
    Ka = np.ascontiguousarray(Ka, dtype=np.float64)
    out = np.zeros(18)
    st = _harness().vch_convert(synth.MODEL_IDS[ma], _p(Ka), len(Ka), size[0], size[1], synth.MODEL_IDS[mb], grid[0], grid[1], C.c_double(fit_radius), int(max_iters),
                                None if start is None else _p(np.ascontiguousarray(start, dtype=np.float64)), C.c_uint(free_mask), _p(out))
    if st != 0:
        return st, None
    return 0, dict(K=out[:cv.NK[mb]].copy(), status=int(out[10]), iterations=int(out[11]), n_fit=int(out[12]), n_left_out=int(out[13]), cost0=out[14], cost=out[15],
                   max_err=out[16], worst=int(out[17]))


def host_run(c):
    st, out = host_convert(c.a, c.mb, c.fit_radius, c.max_iters, c.user_start, c.free_mask, grid=c.grid)
    assert st == 0
    return out


def host_compare(c, Kb):
    ma, Ka = c.a
    Ka, Kb = np.ascontiguousarray(Ka, dtype=np.float64), np.ascontiguousarray(Kb, dtype=np.float64)
    out = np.zeros(4)
    assert _harness().vch_convert_compare(synth.MODEL_IDS[ma], _p(Ka), len(Ka), cv.SIZE[0], cv.SIZE[1], synth.MODEL_IDS[c.mb], _p(Kb), len(Kb), c.grid[0], c.grid[1],
                                          _p(out)) == 0
    return dict(count=int(out[0]), sum_sq=out[1], max_err=out[2], worst=int(out[3]))


# ---------------------------------------------------------------------------------------------------------------- checks 1 - 5 on the host build
@pytest.mark.parametrize("name", cv.case_names())
def test_host_arithmetic(name):
    cv.check_case(name, host_run, host_compare)


def test_one_workgroup_lattice_and_iteration_cap():
    out = host_run(cv.case("same-poly3-one-workgroup"))
    assert out["status"] == 0 and out["n_fit"] == 1024 and out["max_err"] <= cv.ZERO_BOUND
    st, capped = host_convert(("rational6", uc.gt("rational6")), "poly3", max_iters=2)
    assert st == 0 and capped["status"] == 1 and capped["iterations"] == 2 and capped["cost"] < capped["cost0"]


def test_a_start_at_the_optimum_is_converged_without_a_trial():
    K = uc.gt("poly3")
    st, out = host_convert(("poly3", K), "poly3", start=K)
    assert st == 0 and out["status"] == 0 and out["iterations"] == 0 and np.array_equal(out["K"], K) and out["cost"] == out["cost0"]


def test_run_argument_errors_on_the_host_build():
    a = ("poly3", uc.gt("poly3"))
    assert host_convert(a, "kb4", fit_radius=0.0)[0] == -2 and host_convert(a, "kb4", fit_radius=-1.0)[0] == -2
    assert host_convert(a, "kb4", fit_radius=float("nan"))[0] == -2
    bad = np.zeros(8); bad[:4] = a[1][:4]; bad[6] = np.inf
    assert host_convert(a, "kb4", start=bad)[0] == -2
    bad[6] = np.nan
    assert host_convert(a, "kb4", start=bad)[0] == -2
    assert host_convert(a, "kb4", free_mask=1 << 8)[0] == -2 and host_convert(a, "kb4", free_mask=0xff)[0] == 0
    assert host_convert(a, "rational6", grid=(2, 2))[0] == -6                       # 8 residuals, 10 free parameters: VC_ERR_NUMERIC
    assert host_convert(a, "rational6", grid=(2, 2), free_mask=0xf)[0] == 0         # ... and 4 of them
    assert host_convert(a, "kb4", grid=(641, 48))[0] == -2 and host_convert(a, "kb4", grid=(1, 48))[0] == -2
    assert host_convert(("poly3", a[1][:6]), "kb4")[0] == -2


# ---------------------------------------------------------------------------------------------------------------- the handle without a device
def _create(ma, Ka, mb, size, grid):
    h = C.c_void_p()
    Ka = np.ascontiguousarray(Ka, dtype=np.float64)
    st = lib.load().vc_converter_create(0, int(ma), _p(Ka), len(Ka), size[0], size[1], int(mb), grid[0], grid[1], C.byref(h))
    if h.value:
        lib.load().vc_converter_destroy(h)
    return st


def test_argument_errors_come_before_the_device():
    K3 = uc.gt("poly3")
    P3, KB4 = synth.MODEL_IDS["poly3"], synth.MODEL_IDS["kb4"]
    assert _create(P3, K3, 6, (640, 480), (64, 48)) == -2 and _create(P3, K3, -1, (640, 480), (64, 48)) == -2        # an unknown target model
    assert _create(7, K3, KB4, (640, 480), (64, 48)) == -2                        # an unknown source model
    assert _create(P3, K3[:6], KB4, (640, 480), (64, 48)) == -2                   # a wrong nparams
    assert _create(P3, K3, KB4, (640, 480), (641, 48)) == -2                      # a grid above the image
    assert _create(P3, K3, KB4, (640, 480), (64, 481)) == -2
    assert _create(P3, K3, KB4, (640, 480), (1, 48)) == -2
    assert _create(P3, K3, KB4, (4096, 4096), (2049, 2048)) == -2                 # above 2^22 samples
    L = lib.load()
    assert L.vc_convert_run(None, C.c_double(1.0), 0, None, C.c_uint(0)) == -2
    assert L.vc_convert_get(None, None, None, None, None, None, None, None, None, None, None) == -2
    assert L.vc_convert_comparer(None, None) == -2 and L.vc_time_convert(None, 1, None) == -2
    assert L.vc_converter_create_for_camera(None, 0, KB4, 64, 48, None) == -2
    L.vc_converter_destroy(None)


def test_no_cpu_fallback_without_device():
    if _have_gpu():
        pytest.skip("GPU present")
    P3, R6 = synth.MODEL_IDS["poly3"], synth.MODEL_IDS["rational6"]
    assert _create(P3, uc.gt("poly3"), R6, (640, 480), (64, 48)) == -1             # VC_ERR_NO_DEVICE
    assert _create(P3, uc.gt("poly3"), R6, (4096, 4096), (2048, 2048)) == -1       # exactly 2^22 samples is allowed
    with pytest.raises(lib.VicalibError):
        lib.Converter(("poly3", uc.gt("poly3")), "kb4", (640, 480))


# ---------------------------------------------------------------------------------------------------------------- the command line
def _cli(*args):
    return subprocess.run([BIN] + list(args), capture_output=True, text=True, timeout=120)


def _rig(tmp_path):
    Ta, Tb = rc.hand_rig()
    a = tmp_path / "a.xml"
    a.write_text(cc.rig_xml([("poly3", uc.gt("poly3"), Ta), ("kb4", uc.gt("kb4"), Tb)]))
    return a


def test_cli_flag_errors(tmp_path):
    a, out = str(_rig(tmp_path)), str(tmp_path / "converted.xml")
    for args, word in ((["-convert_models", a], "convert_to"),
                       (["-convert_models", a, "-convert_to", "poly4"], "convert_to"),                   # an unknown model
                       (["-convert_models", a, "-convert_to", "poly3,kb4,fov"], "convert_to"),           # neither one model nor the rig's two
                       (["-convert_models", a, "-convert_to", "poly3,"], "convert_to"),
                       (["-convert_models", a, "-convert_to", "kb4", "-convert_grid", "64"], "convert_grid"),
                       (["-convert_models", a, "-convert_to", "kb4", "-convert_grid", "1x48"], "convert_grid"),
                       (["-convert_models", a, "-convert_to", "kb4", "-convert_grid", "641x48"], "convert_grid"),
                       (["-convert_models", a, "-convert_to", "kb4", "-convert_fit_radius", "0"], "convert_fit_radius"),
                       (["-convert_models", a, "-convert_to", "kb4", "-compare_models", a + "," + a, "-compare_dir", str(tmp_path / "cmp")], "exclude"),
                       (["-convert_to", "kb4"], "No camera URI")):
        r = _cli(*(args + ["-convert_output", out]))
        assert r.returncode == 1 and word in r.stderr, (args, r.returncode, r.stderr[-300:])
        assert not os.path.exists(out)
    r = _cli("-convert_models", str(tmp_path / "missing.xml"), "-convert_to", "kb4", "-convert_output", out)
    assert r.returncode == 1 and "cannot open rig file" in r.stderr and not os.path.exists(out)


def test_cli_without_a_device(tmp_path):
    if _have_gpu():
        pytest.skip("GPU present")
    out = tmp_path / "converted.xml"
    r = _cli("-convert_models", str(_rig(tmp_path)), "-convert_to", "kb4,poly3", "-convert_output", str(out))
    assert r.returncode == 3 and "no HIP device" in r.stderr and not out.exists(), (r.returncode, r.stderr[-300:])
