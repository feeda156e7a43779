"""The predicted centre bias of a dot (vc_dot_bias_batch), the part that needs no GPU: its arithmetic (vc_dot_bias.hpp) compiled for the host and
run one observation at a time (tests/host_harness/dot_bias_harness.cpp), held to the numpy reference (tests/dot_bias_ref.py) by the checks of
tests/dot_bias_cases.py, the same checks tests/test_dot_bias_gpu.py applies to the kernel; the entry point's argument errors and its refusal to
run without a device; the Python face's refusals; the command line's flags."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dot_bias_cases as dc
import vicalib_amd.lib as lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")
BAD_ARG, NO_DEVICE = -2, -1


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.parametrize("name", dc.GROUPS)
def test_host_build_matches_the_reference(name):
    dc.check(name, dc.host_run(dc.batch_arrays(dc.group(name))), label=" (host build)")


@pytest.mark.parametrize("n", dc.PREFIXES)
def test_host_build_on_every_batch_shape(n):
    arrays, rows = dc.prefix(n)
    dc.check("models", dc.host_run(arrays), label=" (host build, %d observations)" % n, rows=rows)


def test_host_build_an_observation_does_not_depend_on_the_others():
    full = dc.host_run(dc.batch_arrays(dc.group("models")))
    for k in (0, 3, 4, 100, 256):
        alone = dc.host_run(dc.batch_arrays(dc.group("models"), keep=[k]))
        assert alone["bias"].tobytes() == full["bias"][k:k + 1].tobytes() and alone["radius_px"][0] == full["radius_px"][k]


def _call(n_views=2, device=0, models=None, offsets=None, radii=None, **use):
    L = lib.load()
    names, params, T, o, pw, rad = dc.batch_arrays(dc.group("axis"))
    m, K, T, o, pw, rad = dc.c_arrays(names[:2], params[:2], T[:2], o[:3], pw[:2], rad[:2])
    a = dict(model=m if models is None else np.array(models, dtype=np.int32), K=K, T=T, off=o if offsets is None else np.array(offsets, dtype=np.int32), pw=pw,
             radius=rad if radii is None else np.array(radii, dtype=np.float64), bias=np.zeros((2, 2)), radius_px=np.zeros(2), status=np.zeros(2, dtype=np.int32))
    p = {k: (dc._p(a[k]) if use.get(k, True) else None) for k in a}
    return L.vc_dot_bias_batch(device, n_views, p["model"], p["K"], p["T"], p["off"], p["pw"], p["radius"], p["bias"], p["radius_px"], p["status"])


def test_argument_errors_come_before_the_device():
    for missing in ("model", "K", "T", "off", "pw", "radius", "bias", "radius_px", "status"):
        assert _call(**{missing: False}) == BAD_ARG, missing
    assert _call(n_views=-1) == BAD_ARG
    assert _call(offsets=[0, 2, 1]) == BAD_ARG and _call(offsets=[-1, 0, 1]) == BAD_ARG                      # offsets that decrease; a negative start
    assert _call(models=[0, 6]) == BAD_ARG and _call(models=[-1, 0]) == BAD_ARG                        # an unknown model
    for r in (-1e-3, float("nan"), float("inf")):
        assert _call(radii=[0.0094, r]) == BAD_ARG, r
    assert _call(device=-1, n_views=-1) == BAD_ARG                                                   # (the arguments are judged before the device)
    L = lib.load()
    ms = C.c_double(0)
    m, K, T, o, pw, rad = dc.c_arrays(*dc.batch_arrays(dc.group("axis")))
    time = lambda reps, out, radius=rad, n=6: L.vc_time_dot_bias_batch(0, n, dc._p(m), dc._p(K), dc._p(T), dc._p(o), dc._p(pw), dc._p(radius), reps, out)
    assert time(0, C.byref(ms)) == BAD_ARG and time(3, None) == BAD_ARG and time(3, C.byref(ms), radius=-rad) == BAD_ARG and time(3, C.byref(ms), n=0) == BAD_ARG
    if not _have_gpu():          # no host fallback: a valid call without a device is refused
        assert _call() == NO_DEVICE and _call(n_views=0) == NO_DEVICE and time(3, C.byref(ms)) == NO_DEVICE


def test_python_face_refuses_what_the_library_refuses():
    models, params, T, off, pw, rad = dc.batch_arrays(dc.group("axis"))
    with pytest.raises(lib.VicalibError):
        lib.dot_bias_batch(models, params, T, off[:-1], pw, rad)                   # one offset short
    with pytest.raises(lib.VicalibError):
        lib.dot_bias_batch(models, params, T, off, pw, rad[:-1])                   # radii and centres disagree
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        lib.dot_bias_batch(models, params, T, off, pw, -rad)
    if not _have_gpu():
        with pytest.raises(lib.VicalibError, match="NO_DEVICE"):
            lib.dot_bias_batch(models, params, T, off, pw, rad)
        with pytest.raises(lib.VicalibError, match="NO_DEVICE"):
            lib.time_dot_bias_batch(models, params, T, off, pw, rad, reps=2)


def test_help_lists_the_flags():
    r = subprocess.run([BIN, "-help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    for flag in ("-dot_bias_rounds", "-dot_radius", "-grid_large_rad", "-grid_small_rad"):
        assert flag in text, flag


@pytest.mark.parametrize("extra, word", [(["-gpus", "2"], "-gpus"), (["-holdout_every", "5"], "-holdout_every"), (["-dot_bias_rounds", "-1"], "dot_bias_rounds"),
                                         (["-dot_radius", "-0.01"], "dot_radius")])
def test_flag_errors_come_before_anything_runs(tmp_path, extra, word):
    """exit status 1 and the flags' names, with or without a GPU, and nothing read or written"""
    out = tmp_path / "cameras.xml"
    args = [BIN, "-cam", "detections://" + str(tmp_path / "none.csv"), "-models", "linear", "-output", str(out)]
    args += ([] if extra[0] == "-dot_bias_rounds" else ["-dot_bias_rounds", "1"]) + extra
    r = subprocess.run(args, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == 1 and word in r.stderr and "dot_bias_rounds" in r.stderr, r.stdout + r.stderr
    assert "none.csv" not in r.stderr and not out.exists()
