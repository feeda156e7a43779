"""The device build of the camera models at their branch points (vc_math.hpp under __HIP_DEVICE_COMPILE__: v_rcp_f64 / v_rsq_f64 with two
Newton steps, fast_sqrt_rsqrt(0) leaving a NaN that only the selects of project_radial and project_kb4 keep out, contraction to FMA,
the device math library's tan) against the mpmath reference of tests/golden/model_edges.json -- corners on the axis, radii from 1e-9 to
90 on both sides of every threshold, fov's w on both sides of its own, kb4 at and beyond 90 degrees, 2^40 and 2^-40, detections from
exact to 1e6 px off.  No device code is added for this: every number is read through faces the solver already has.

Pixel face: with a detection of (0, 0) the residual of the report's sweep is project_any<false> itself; vc_evaluate's cost and sum of
squares are the sweep the LM loop decides with.  Gram face: vc_linearize on two 8-corner frames per camera (project_any<true>,
corner_rows, the tile Gram, tile_to_frame_blocks, the camera block): H_pp and g_p per frame, hss_diag and g_s, the cost.  A camera
whose w column is identically zero (w*w <= 1e-5) has its intrinsics fixed.  Every read-out must be finite; where the reference is
exactly zero or exactly the principal point, so is the device.  Bounds and scales: model_edges_cases.py.

Measured on the MI355X (DESIGN.md section 5 has the table): pixel 2.4e-15, H_pp 6.4e-15, g_p 4.2e-16, hss_diag 3.6e-15 (w column 4.5e-11
at w = 0.00317), g_s 1.5e-16, cost 1.5e-15.  With irho for irho1 in project_kb4 the axis pixel is NaN, with fast_rcp's raw estimate the
pixels are off by 7e-10 and more: both fail here and pass everywhere else.  One Newton step instead of two does NOT fail, at these or
any honest bounds: it moves the result by under an ulp (largest pixel deviation 2.4e-15 -> 2.6e-15)."""
import numpy as np
import pytest

import model_edges_cases as mc
from vicalib_amd.lib import ViCalibrator

pytestmark = pytest.mark.gpu


def _calibrator(cam):
    cal = ViCalibrator(0)
    cal.AddCamera(cam["model"], cam["k"], mc.IDENTITY)
    cal.SetCalibrateImu(False)
    if cam["fix_k"]:
        cal.FixCameraIntrinsics(True)
    return cal


@pytest.mark.parametrize("name", mc.camera_names())
def test_device_projection_matches_the_reference(name):
    cam = mc.camera(name)
    cal = _calibrator(cam)
    n = len(cam["p"])
    for f, lo in enumerate(range(0, n, 8)):
        cal.AddFrame(mc.IDENTITY, 0.05 * f)
        cal.AddObservations(f, 0, cam["p"][lo:lo + 8], np.zeros((len(cam["p"][lo:lo + 8]), 2)))
    cal.prepare()        # (sets the residual multiplicity to one, as linearize() does: a report's own upload leaves it at zero, and the cost with it)
    rep = cal.report(bins=(1, 1))
    assert rep["r"].shape == (n, 2)
    cost, sq = cal.evaluate()
    mx = mc.Maxima(); bad = []
    for i, tag in enumerate(cam["tags"]):
        what = "%s %s" % (name, tag)
        if not mx.add("pixel", mc.dev_pixel(rep["r"][i][None, :], cam["pix"][i][None, :], cam["k"], what), mc.PIXEL_BOUND, what):
            bad.append(what)
    ok_cost = mx.add("sweep cost", mc.dev_cost(cost, cam["pixel_cost"], name), mc.COST_BOUND, name)
    ok_sq = mx.add("sweep sum of squares", mc.dev_cost(sq, cam["pixel_sum_sq"], name), mc.COST_BOUND, name)
    print("\n".join(mx.lines()))
    assert not bad and ok_cost and ok_sq, (bad, mx.lines())
    cal.close()


@pytest.mark.parametrize("name", mc.camera_names())
def test_device_gram_blocks_match_the_reference(name):
    cam = mc.camera(name)
    cal = _calibrator(cam)
    for f, fr in enumerate(cam["frames"]):
        cal.AddFrame(mc.IDENTITY, 0.05 * f)
        cal.AddObservations(f, 0, fr["pw"], fr["uv"])
    g = cal.linearize()
    nk = 0 if cam["fix_k"] else cam["nk"]
    assert cal.shared_dim() == nk and g["Hpp"].shape == (2, 6, 6)
    for key in ("Hpp", "gp", "S", "g_red", "hss_diag", "g_s"):
        assert np.all(np.isfinite(g[key])), (key, g[key])
    mx = mc.Maxima(); ok = True
    for f, fr in enumerate(cam["frames"]):
        what = "%s frame %s" % (name, fr["tag"])
        ok &= mx.add("H_pp", mc.dev_H(g["Hpp"][f], fr["Hpp"], what), mc.H_BOUND, what)
        ok &= mx.add("g_p", mc.dev_g(g["gp"][f], fr["gp"], np.diag(fr["Hpp"]), fr["cost"], what), mc.G_BOUND, what)
    ok &= mx.add("cost", mc.dev_cost(g["cost"], cam["cost"], name), mc.COST_BOUND, name)
    if nk:
        _, col = mc.w_factor(cam)
        hb = mc.k_bounds(cam, mc.H_BOUND, 1); gb = mc.k_bounds(cam, mc.G_BOUND, 1)
        dh = mc.dev_H(g["hss_diag"], cam["hss_diag"], name); dg = mc.dev_g(g["g_s"], cam["g_s"], cam["hss_diag"], cam["cost"], name)
        rest = np.arange(nk) != col
        ok &= mx.add("hss_diag", dh[rest], hb[rest], name) & mx.add("g_s", dg[rest], gb[rest], name)
        ok &= mx.add("hss_diag, fov w column", dh[~rest], hb[~rest], name) & mx.add("g_s, fov w column", dg[~rest], gb[~rest], name)
    print("\n".join(mx.lines()))
    assert ok, mx.lines()
    cal.close()
