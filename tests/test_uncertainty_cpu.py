"""Mapping the projection uncertainty of a calibrated camera (vc_uncertainty*), the part that needs no GPU: the map's arithmetic
(vc_uncertainty.hpp) compiled for the host and held to the same numpy reference and the same checks that tests/test_uncertainty_gpu.py applies
to the kernels, the semantic pin against a numpy comparison of K with K + delta e_k, the exact properties, argument errors, the refusal to run
without a device, and the command line's flag errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import uncertainty_cases as un
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
    src = os.path.join(HERE, "host_harness", "uncertainty_harness.cpp")
    so = os.path.join(HERE, "host_harness", "libvc_uncertainty_harness.so")
    deps = [src] + [os.path.join(ROOT, "vicalib_amd", "csrc", f) for f in ("vc_uncertainty.hpp", "vc_convert.hpp", "vc_lm_rules.hpp", "vc_compare.hpp", "vc_rectify.hpp",
                                                                          "vc_undistort.hpp", "vc_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_uncertainty(camera, cov, sigma_px=1.0, fit_radius=0.5, size=un.SIZE, grid=un.GRID, ring_counts=un.RING_COUNTS):
    """the host build of a whole run; (status, dict in the layout the checks take)"""
    m, K = camera
    K = np.ascontiguousarray(K, dtype=np.float64)
    cov = np.ascontiguousarray(cov, dtype=np.float64)
    n, nk = grid[0] * grid[1], len(K)
    out = None
    for nr in ring_counts:
        fit, sg, fl, summary, rings = np.zeros(40), np.zeros((n, 3)), np.zeros(n, dtype=np.uint8), np.zeros(5), np.zeros((nr, 4))
        st = _harness().vch_uncertainty(synth.MODEL_IDS[m], _p(K), nk, size[0], size[1], grid[0], grid[1], _p(cov), C.c_double(sigma_px), C.c_double(fit_radius), int(nr),
                                        _p(fit), _p(sg), _p(fl), _p(summary), _p(rings))
        if st != 0:
            return st, None
        if out is None:
            out = dict(M=fit[:3 * nk].reshape(3, nk).copy(), G=fit[30:39].reshape(3, 3).copy(), n_fit=int(fit[39]), sigma=sg, flags=fl, rings={},
                       summary=dict(count=int(summary[0]), invalid=int(summary[1]), sum_var=summary[2], max_lam=summary[3], worst=int(summary[4])))
        out["rings"][nr] = dict(count=rings[:, 0].astype(np.int64), invalid=rings[:, 1].astype(np.int64), sum_var=rings[:, 2].copy(), max_lam=rings[:, 3].copy())
    return 0, out


def host_run(c, cov, sigma_px, fit_radius):
    st, out = host_uncertainty(c.camera, cov, sigma_px, fit_radius, grid=c.grid)
    assert st == 0
    return out


def host_args_ok(cov, nk, sigma_px=1.0, fit_radius=0.5):
    cov = np.ascontiguousarray(cov, dtype=np.float64)
    return bool(_harness().vch_uncertainty_args_ok(_p(cov), int(nk), C.c_double(sigma_px), C.c_double(fit_radius)))


# ---------------------------------------------------------------------------------------------------------------- checks 1 and 2 on the host build
_deviations = {}


@pytest.mark.parametrize("name", un.case_names())
def test_host_arithmetic(name):
    _, dev = un.check_case(name, host_run)
    _deviations[name] = dev
    print("largest relative deviation of the host harness from numpy so far: %.3g (uncertainty_cases.MEASURED = %.3g)" % (max(_deviations.values()), un.MEASURED))


def test_beyond_has_invalid_samples_and_a_clean_fit_set():
    ref, c = un.reference("beyond"), un.case("beyond")
    out = host_run(c, c.cov, 1.0, c.fit_radius)
    assert out["summary"]["invalid"] > 0.5 * len(ref.q) and 0 < ref.undecided.sum() <= 0.1 * len(ref.q)
    assert out["n_fit"] == (ref.rho <= c.fit_radius).sum()


# ---------------------------------------------------------------------------------------------------------------- check 3: the semantic pin
@pytest.mark.parametrize("model,k,delta,tabulated", un.PIN)
def test_rank_one_covariance_is_the_comparers_difference(model, k, delta, tabulated):
    d, w, gap = un.pin_numpy(model, k, delta)
    _, _, half = un.pin_numpy(model, k, 0.5 * delta)
    print("%s parameter %d: gap %.3g px at delta, %.3g px at delta / 2: ratio %.3f" % (model, k, gap, half, gap / half))
    assert 3.5 <= gap / half <= 4.5                                 # second order in delta
    st, out = host_uncertainty((model, uc.gt(model)), un.pin_cov(model, k, delta), 1.0, un.PIN_FIT_RADIUS)
    assert st == 0
    un.check_pin(model, k, delta, tabulated, out, d, w)


# ---------------------------------------------------------------------------------------------------------------- check 4: exact properties
def test_exact_properties_on_the_host_build():
    c = un.case("kb4-0.5")
    one = host_run(c, c.cov, 1.0, 0.5)
    zero = host_run(c, np.zeros_like(c.cov), 1.0, 0.5)
    assert not np.any(zero["sigma"]) and np.array_equal(zero["flags"], one["flags"]) and zero["summary"]["sum_var"] == 0 and zero["summary"]["max_lam"] == 0
    assert un.same_bits(one, host_run(c, c.cov, 2.0, 0.5), scale=4.0)
    assert un.same_bits(one, host_run(c, c.cov, 1.0, 0.5))
    plain = host_run(c, c.cov, 1.0, 0.0)
    assert not np.any(plain["M"]) and plain["n_fit"] == 0
    assert un.same_bits(plain, host_run(c, c.cov, 1.0, -1.0))


def test_lattice_sizes_and_too_small_a_fit_set():
    c = un.case("tiny")
    st, out = host_uncertainty(c.camera, c.cov, 1.0, 1.0, grid=un.TINY)
    assert st == 0 and out["n_fit"] == 4 and out["summary"]["count"] == 4
    assert host_uncertainty(c.camera, c.cov, 1.0, 0.5, grid=un.TINY)[0] == -6          # no corner within half the half-diagonal: VC_ERR_NUMERIC
    st, out = host_uncertainty(c.camera, c.cov, 1.0, 1.0, grid=un.ONE_WORKGROUP)
    assert st == 0 and out["n_fit"] == 1024


def test_run_argument_errors_through_the_shared_check():
    cov = un.dense_cov("poly3")
    assert host_args_ok(cov, 7) and host_args_ok(np.zeros((7, 7)), 7) and host_args_ok(cov, 7, fit_radius=0.0) and host_args_ok(cov, 7, fit_radius=-1.0)
    bad = cov.copy(); bad[1, 4] += 1e-9
    assert not host_args_ok(bad, 7)                                 # not symmetric
    ok = cov.copy(); ok[1, 4] += 1e-14 * cov.diagonal().max()
    assert host_args_ok(ok, 7)                                      # ... symmetric to 1e-12 max |diag|
    bad = cov.copy(); bad[3, 3] = -1e-6
    assert not host_args_ok(bad, 7)                                 # a negative diagonal entry
    for v in (np.nan, np.inf):
        bad = cov.copy(); bad[2, 5] = bad[5, 2] = v
        assert not host_args_ok(bad, 7)
    for s in (0.0, -1.0, np.nan, np.inf):
        assert not host_args_ok(cov, 7, sigma_px=s)
    assert not host_args_ok(cov, 7, fit_radius=np.nan)
    a = ("poly3", uc.gt("poly3"))
    bad = cov.copy(); bad[0, 1] += 1.0
    assert host_uncertainty(a, bad)[0] == -2 and host_uncertainty(a, cov, sigma_px=0.0)[0] == -2
    assert host_uncertainty(a, cov, grid=(641, 48))[0] == -2 and host_uncertainty(a, cov, grid=(1, 48))[0] == -2
    assert host_uncertainty(("poly3", a[1][:6]), cov[:6, :6])[0] == -2


# ---------------------------------------------------------------------------------------------------------------- the handle without a device
def _create(m, K, size, grid):
    h = C.c_void_p()
    K = np.ascontiguousarray(K, dtype=np.float64)
    st = lib.load().vc_uncertainty_create(0, int(m), _p(K), len(K), size[0], size[1], grid[0], grid[1], C.byref(h))
    if h.value:
        lib.load().vc_uncertainty_destroy(h)
    return st


def test_argument_errors_come_before_the_device():
    K3 = uc.gt("poly3")
    P3 = synth.MODEL_IDS["poly3"]
    assert _create(7, K3, (640, 480), (64, 48)) == -2 and _create(-1, K3, (640, 480), (64, 48)) == -2        # an unknown model
    assert _create(P3, K3[:6], (640, 480), (64, 48)) == -2                   # a wrong nparams
    assert _create(P3, K3, (640, 480), (641, 48)) == -2                      # a grid above the image
    assert _create(P3, K3, (640, 480), (64, 481)) == -2
    assert _create(P3, K3, (640, 480), (1, 48)) == -2
    assert _create(P3, K3, (4096, 4096), (2049, 2048)) == -2                 # above 2^22 samples
    L = lib.load()
    assert L.vc_uncertainty_create(0, P3, _p(K3), 7, 640, 480, 64, 48, None) == -2
    assert L.vc_uncertainty_run(None, None, C.c_double(1.0), C.c_double(0.5)) == -2
    assert L.vc_uncertainty_get_fit(None, None, None, None) == -2 and L.vc_uncertainty_get_map(None, None, None) == -2
    assert L.vc_uncertainty_summary(None, None, None, None, None, None) == -2 and L.vc_uncertainty_rings(None, 8, None, None, None, None) == -2
    assert L.vc_time_uncertainty(None, 1, None) == -2
    assert L.vc_uncertainty_create_for_camera(None, 0, 64, 48, None) == -2
    L.vc_uncertainty_destroy(None)


def test_no_cpu_fallback_without_device():
    if _have_gpu():
        pytest.skip("GPU present")
    P3 = synth.MODEL_IDS["poly3"]
    assert _create(P3, uc.gt("poly3"), (640, 480), (64, 48)) == -1             # VC_ERR_NO_DEVICE
    assert _create(P3, uc.gt("poly3"), (4096, 4096), (2048, 2048)) == -1       # exactly 2^22 samples is allowed
    with pytest.raises(lib.VicalibError):
        lib.Uncertainty(("poly3", uc.gt("poly3")), (640, 480))


# ---------------------------------------------------------------------------------------------------------------- the command line
def test_cli_flag_errors(tmp_path):
    out = str(tmp_path / "unc")
    for args, word in ((["-uncertainty_grid", "64"], "uncertainty_grid"),
                       (["-uncertainty_grid", "1x48"], "uncertainty_grid"),
                       (["-uncertainty_rings", "0"], "uncertainty_rings"),
                       (["-uncertainty_rings", "65"], "uncertainty_rings"),
                       (["-uncertainty_noise", "-1"], "uncertainty_noise")):
        r = subprocess.run([BIN, "-cam", "detections://missing.txt", "-uncertainty_dir", out] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and word in r.stderr, (args, r.returncode, r.stderr[-300:])
        assert not os.path.exists(out)
