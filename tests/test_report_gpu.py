"""The residual report (vc_report_*: per corner, per view, per image cell, per IMU block) through the C ABI, against the CPU oracle at
identical parameters and against numpy restatements of its own sums.  Tolerances are the project's: 1e-6 relative with an absolute floor
of 1e-9 against the oracle (north_star; _compare_solution's floor), 1e-12 relative for sums that repeat the solver's own arithmetic."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import holdout_cases as hc
import oracle_lib as ol
from vicalib_amd import synth
from vicalib_amd.lib import ViCalibrator

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps
ALL_MODELS = ["fov", "poly2", "poly3", "kb4", "linear", "rational6"]


def _load_pair(p, calibrate_imu=False, **orc_opts):
    """The problem's tiles, in order, into a calibrator and an oracle; returns them with the corners' (frame, camera, dot, pixel) in the
    caller's order."""
    cal = ViCalibrator(0); orc = ol.Oracle()
    for c, m in enumerate(p.cam_model):
        cal.AddCamera(m, p.cam_K_init[c], p.cam_T_ck_init[c], p.cfg.width, p.cfg.height)
        orc.add_camera(m, p.cam_K_init[c], p.cam_T_ck_init[c], p.cfg.width, p.cfg.height)
    for n in range(len(p.frame_time)):
        cal.AddFrame(p.frame_T_wk_init[n], p.frame_time[n]); orc.add_frame(p.frame_T_wk_init[n], p.frame_time[n])
    fr, cm, dot, pix = [], [], [], []
    for (f, c, ids, px) in p.tiles:
        cal.AddObservations(f, c, p.grid_points[ids], px); orc.add_observations(f, c, p.grid_points[ids], px)
        fr += [f] * len(ids); cm += [c] * len(ids); dot += list(ids); pix.append(np.asarray(px, dtype=np.float64).reshape(-1, 2))
    if p.imu_t is not None:
        cal.AddImuMeasurements(p.imu_gyro, p.imu_accel, p.imu_t); orc.add_imu(p.imu_gyro, p.imu_accel, p.imu_t)
    cal.SetCalibrateImu(calibrate_imu)
    orc.set_options(calibrate_imu=calibrate_imu, **orc_opts)
    corners = dict(frame=np.array(fr, dtype=np.int32), camera=np.array(cm, dtype=np.int32), dot=np.array(dot), pix=np.concatenate(pix) if pix else np.zeros((0, 2)))
    return cal, orc, corners


def _oracle_takes_state(orc, cal, imu=False):
    for c in range(cal.NumCameras()):
        K, T = cal.GetCamera(c)
        orc.set_camera(c, K, T)
    for f in range(cal.NumFrames()):
        T, v, _ = cal.GetFrame(f)
        orc.set_frame(f, T, v if imu else None)
    if imu:
        orc.set_imu_state(cal.GetBiases(), cal.GetScaleFactor(), cal.GetGravity(), cal.time_offset())


def _view_order(frame, camera):
    """Stable order by (frame, camera): position inside a view is the order of arrival."""
    return np.lexsort((np.arange(len(frame)), camera, frame))


def _check_corners_against_oracle(rep, orc):
    ro, fo, co = orc.residuals()
    a = _view_order(rep["frame"], rep["camera"]); b = _view_order(fo, co)
    np.testing.assert_array_equal(rep["frame"][a], fo[b])
    np.testing.assert_array_equal(rep["camera"][a], co[b])
    err = np.abs(rep["r"][a] - ro[b]); bound = 1e-6 * np.abs(ro[b]) + 1e-9
    print("corners vs oracle: max |r_gpu - r_oracle| = %.3e px, max of error / bound = %.3e" % (err.max(), (err / bound).max()))
    assert np.all(err <= bound)


def _check_views(rep, cal=None):
    """Every view row from the report's own corner residuals."""
    r, fl = rep["r"], rep["flags"]
    v = rep["views"]
    in_problem = (fl & 1) == 0
    mag = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])
    keys = sorted(set(zip(rep["frame"].tolist(), rep["camera"].tolist())))
    assert list(zip(v["frame"].tolist(), v["camera"].tolist())) == keys
    worst_rel = 0.0
    for i, (f, c) in enumerate(keys):
        idx = np.nonzero((rep["frame"] == f) & (rep["camera"] == c))[0]
        live = idx[in_problem[idx]]
        assert v["count"][i] == len(live)
        assert v["removed"][i] == int(np.count_nonzero(fl[idx]))
        sq = float((mag[live] ** 2).sum()) if len(live) else 0.0
        ref_sq = float((r[live, 0] * r[live, 0] + r[live, 1] * r[live, 1]).sum()) if len(live) else 0.0
        assert abs(v["sum_sq"][i] - ref_sq) <= 1e-12 * max(ref_sq, sq)
        if len(live):
            w = live[np.argmax(mag[live])]            # (argmax: the first, i.e. lowest, index on ties)
            assert v["worst_corner"][i] == w
            # 1e-15 relative, not bitwise: |r| is a square root taken on the device; the radicand is formed without contraction, exactly as
            # numpy forms it, but the device's double-precision square root is specified to 1 ulp, numpy's is correctly rounded
            worst_rel = max(worst_rel, abs(v["max_err"][i] - mag[w]) / mag[w])
            assert abs(v["max_err"][i] - mag[w]) <= 1e-15 * mag[w]
        else:
            assert v["worst_corner"][i] == -1 and v["max_err"][i] == 0.0
    print("views: %d rows, max relative difference of max_err to numpy's |r| = %.3e" % (len(keys), worst_rel))
    if cal is not None:
        for c in range(cal.NumCameras()):
            m = v["camera"] == c
            rmse = np.sqrt(v["sum_sq"][m].sum() / (2.0 * v["count"][m].sum()))
            assert abs(rmse - cal.GetCameraProjRMSE()[c]) <= 1e-12 * rmse
        assert abs(v["sum_sq"].sum() - cal.evaluate()[1]) <= 1e-12 * v["sum_sq"].sum()


def _numpy_maps(rep, pix, width, height, n_cams):
    bx, by = rep["bins"]
    ix = np.clip(np.floor(pix[:, 0] * bx / width), 0, bx - 1).astype(int)
    iy = np.clip(np.floor(pix[:, 1] * by / height), 0, by - 1).astype(int)
    live = (rep["flags"] & 1) == 0
    r = rep["r"]
    vals = np.stack([np.ones(len(r)), r[:, 0], r[:, 1], r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]], axis=1)
    maps = np.zeros((n_cams, by, bx, 4)); mabs = np.zeros((n_cams, by, bx, 4))
    for k in np.nonzero(live)[0]:
        maps[rep["camera"][k], iy[k], ix[k]] += vals[k]; mabs[rep["camera"][k], iy[k], ix[k]] += np.abs(vals[k])
    return maps, mabs


def _check_maps(rep, pix, width, height, n_cams):
    maps, mabs = _numpy_maps(rep, pix, width, height, n_cams)
    got = rep["maps"]
    np.testing.assert_array_equal(got[..., 0], maps[..., 0])
    bound = maps[..., :1] * EPS * mabs[..., 1:]            # n_cell * eps * sum |x_i|: a floating-point sum in any order
    err = np.abs(got[..., 1:] - maps[..., 1:])
    print("error map: %d occupied cells, max of error / bound = %.3e" % (np.count_nonzero(maps[..., 0]), (err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound)


def _same_report(a, b):
    for k in ("r", "frame", "camera", "flags", "maps"):
        np.testing.assert_array_equal(a[k], b[k])
    for k in a["views"]:
        np.testing.assert_array_equal(a["views"][k], b["views"][k])
    for k in a["imu"]:
        np.testing.assert_array_equal(a["imu"][k], b["imu"][k])


@pytest.mark.parametrize("model", ALL_MODELS)
def test_corners_views_and_maps_against_the_oracle_at_the_start_and_after_a_solve(model):
    """Items 1, 2, 5 on a two-camera rig of every model, with the generator's missing-detection cases: a frame one camera does not see,
    a frame nobody sees, a view of 5 corners and one of 65 (a ragged second sweep of the wavefront)."""
    p = synth.generate(synth.Config(models=(model, model), n_frames=12, seed=9))
    p.tiles = [t for t in p.tiles if not (t[0] == 3) and not (t[0] == 5 and t[1] == 1)]
    f, c, ids, pix = p.tiles[0]; p.tiles[0] = (f, c, ids[:5], pix[:5])
    f, c, ids, pix = p.tiles[1]; p.tiles[1] = (f, c, ids[:65], pix[:65])
    p.flat = None
    cal, orc, corners = _load_pair(p)
    # start state
    rep = cal.report()
    np.testing.assert_array_equal(rep["frame"], corners["frame"]); np.testing.assert_array_equal(rep["camera"], corners["camera"])
    assert not rep["flags"].any() and len(rep["imu"]["flags"]) == 0
    orc.prepare(vis_mult=1)
    _check_corners_against_oracle(rep, orc)
    _check_views(rep)
    _check_maps(rep, corners["pix"], p.cfg.width, p.cfg.height, 2)
    _same_report(rep, cal.report())
    # after a solve
    cal.SetMaxIters(25); cal.Solve()
    rep = cal.report()
    _oracle_takes_state(orc, cal); orc.prepare(vis_mult=1)
    _check_corners_against_oracle(rep, orc)
    _check_views(rep, cal)
    _check_maps(rep, corners["pix"], p.cfg.width, p.cfg.height, 2)
    _same_report(rep, cal.report())
    # one cell per camera = the camera's totals
    one = cal.report(bins=(1, 1))
    for cam in range(2):
        m = rep["views"]["camera"] == cam
        assert one["maps"][cam, 0, 0, 0] == rep["views"]["count"][m].sum()
        assert abs(one["maps"][cam, 0, 0, 3] - rep["views"]["sum_sq"][m].sum()) <= 1e-12 * one["maps"][cam, 0, 0, 3]
        live = rep["camera"] == cam
        s = rep["r"][live].sum(axis=0); sa = np.abs(rep["r"][live]).sum(axis=0)
        assert np.all(np.abs(one["maps"][cam, 0, 0, 1:3] - s) <= live.sum() * EPS * sa)


def test_the_worst_corner_of_a_view_is_the_lowest_index_among_equal_ones():
    """vc_report.hpp's promise for view_worst: one camera, two frames, the first view cut to 130 corners (two full sweeps of the wavefront
    and a tail) of which the first, the 66th and the last are one target point at one pixel 5 px off -- three bit-equal residuals, the
    largest of the view at the ground-truth start state (detection noise 0.1 px)."""
    p = synth.generate(synth.Config(models=("poly3",), n_frames=2, seed=13))
    f, c, ids, pix = p.tiles[0]
    p.tiles[0] = (f, c) + hc.three_equal_corners(ids, pix)
    p.flat = None
    cal = ViCalibrator(0).load_problem(p, init=False); cal.SetCalibrateImu(False)
    rep = cal.report()
    r, v = rep["r"], rep["views"]
    mag = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])
    trio = [0, 65, 129]
    assert (rep["frame"][129], rep["camera"][129]) == (f, c) == (v["frame"][0], v["camera"][0]) and v["count"][0] == 130
    print("planted |r| = %.6f px (x3), largest other of the view %.6f px" % (mag[0], np.delete(mag[:130], trio).max()))
    np.testing.assert_array_equal(r[trio], np.tile(r[0], (3, 1)))
    assert np.all(np.delete(mag[:130], trio) < mag[0])
    assert v["worst_corner"][0] == 0
    assert abs(v["max_err"][0] - mag[0]) <= 1e-15 * mag[0]            # (the device's square root: see _check_views)
    _check_views(rep)


def test_reading_needs_a_current_report_and_bins_in_range():
    p = synth.generate(synth.Config(models=("poly3",), n_frames=6, seed=3))
    cal = ViCalibrator(0).load_problem(p); cal.SetCalibrateImu(False)
    L = cal.L
    assert L.vc_report_num_views(cal.h) == -2                     # VC_ERR_BAD_ARG before any compute
    for bx, by in [(0, 4), (33, 1), (4, 0), (1, 33), (-1, 3)]:
        assert L.vc_report_compute(cal.h, bx, by) == -2
    rep = cal.report(bins=(32, 32))
    assert rep["maps"].shape == (1, 32, 32, 4) and L.vc_report_num_views(cal.h) == len(p.tiles)
    T = p.frame_T_wk_init[0]
    cal.SetFramePose(0, T)                                          # the problem changed: no stale rows
    assert L.vc_report_num_views(cal.h) == -2 and L.vc_report_num_corners(cal.h) == -2
    cal.report()
    cal.Solve()                                                    # the state moved
    assert L.vc_report_num_views(cal.h) == -2
    cal.report()
    cal.Clear()
    assert L.vc_report_num_views(cal.h) == -2


def _plant_noisy_view(p, view=20, seed=3, sigma=1.0):
    f, c, ids, pix = p.tiles[view]
    pix += np.random.RandomState(seed).normal(size=pix.shape) * sigma       # (in place: `flat` of a native problem sees it too)
    return f, c


def _view_rmse(frame, camera, r, live):
    out = {}
    for f, c in sorted(set(zip(frame.tolist(), camera.tolist()))):
        m = (frame == f) & (camera == c) & live
        if m.any():
            out[(f, c)] = float(np.sqrt((r[m] ** 2).sum() / (2.0 * m.sum())))
    return out


def test_a_planted_bad_view_is_found():
    """Item 3: cfg1 with sigma-1 px noise on every corner of view 20.  Condition on the input, checked with the oracle alone: at its
    solution the planted view's RMSE is at least twice the next largest."""
    p = synth.generate(synth.BASELINE_CONFIGS["cfg1"])
    assert len(p.tiles) == 50 and p.n_obs == 8055
    f20, c20 = _plant_noisy_view(p)
    cal, orc, corners = _load_pair(p)
    orc.solve()
    ro, fo, co = orc.residuals()
    per = _view_rmse(fo, co, ro, np.ones(len(ro), dtype=bool))
    others = max(v for k, v in per.items() if k != (f20, c20))
    print("oracle: planted view %.3f px, next largest %.3f px" % (per[(f20, c20)], others))
    assert per[(f20, c20)] >= 2.0 * others
    cal.Solve()
    v = cal.report()["views"]
    rmse = np.sqrt(v["sum_sq"] / (2.0 * v["count"]))
    k = int(np.argmax(rmse))
    assert (v["frame"][k], v["camera"][k]) == (f20, c20)
    assert rmse[k] >= 2.0 * np.delete(rmse, k).max()


def _plant_outliers(p, shift=25.0):
    planted = []
    for k in range(10):
        f, c, ids, pix = p.tiles[3 + 4 * k]
        d = (5 * k) % len(ids)
        pix[d] += shift * np.array([np.cos(0.7 * k), np.sin(0.7 * k)])
        planted.append((f, c, int(ids[d])))
    return planted


def _planted_mask(corners, planted):
    m = np.zeros(len(corners["frame"]), dtype=bool)
    for (f, c, dot) in planted:
        m |= (corners["frame"] == f) & (corners["camera"] == c) & (corners["dot"] == dot)
    assert m.sum() == len(planted)
    return m


def test_removed_corners_are_reported_vision_only():
    """Item 4, first case: cfg1, 10 corners moved by 25 px, outlier stage at 2 x RMSE.  A one-stage vision-only solve DROPS them (no copy
    left, they leave the device's corner arrays): the report still evaluates them.  Condition, with the oracle solved without outlier
    removal: |r| > 2 x camera RMSE holds for exactly the planted corners."""
    p = synth.generate(synth.BASELINE_CONFIGS["cfg1"])
    planted = _plant_outliers(p)
    cal, orc, corners = _load_pair(p)
    want = _planted_mask(corners, planted)
    orc.solve()
    ro, fo, co = orc.residuals()
    mag_o = np.sqrt((ro ** 2).sum(axis=1))
    a = _view_order(corners["frame"], corners["camera"]); b = _view_order(fo, co)
    over = np.zeros(len(mag_o), dtype=bool); over[a] = mag_o[b] > 2.0 * orc.rmse()[0]
    print("oracle: camera RMSE %.3f px, planted |r| %.1f..%.1f px, largest other %.2f px" % (orc.rmse()[0], mag_o[b][want[a]].min(), mag_o[b][want[a]].max(), mag_o[b][~want[a]].max()))
    np.testing.assert_array_equal(over, want)
    cal.SetRemoveOutliers(True, 2.0); cal.Solve()
    rep = cal.report()
    np.testing.assert_array_equal(rep["flags"] != 0, want)
    assert np.all(rep["flags"][want] == 1)                         # dropped
    mag = np.sqrt((rep["r"] ** 2).sum(axis=1))
    assert np.all(mag[want] > 20.0)
    _check_views(rep, cal)                                         # removed counts, sums without the dropped corners, RMSE
    assert rep["views"]["removed"].sum() == 10 and rep["views"]["count"].sum() == len(want) - 10
    _check_maps(rep, corners["pix"], p.cfg.width, p.cfg.height, 1)
    _oracle_takes_state(orc, cal); orc.prepare(vis_mult=1)
    _check_corners_against_oracle(rep, orc)                        # the dropped ones too: the oracle here still holds every corner


VI_CFG = dict(models=("kb4",), n_frames=60, imu=True, seed=5)          # the mono_kb4_imu_60 problem


def test_removed_corners_are_reported_visual_inertial():
    """Item 4, second case: with the IMU the outlier stage leaves a marked corner one copy fewer (bit 1): it stays in its view's count and
    sums, and `removed` counts it.  Condition, with the oracle run through the same stages without outlier removal (the state at which
    the outlier stage runs): |r| > 2 x camera RMSE holds for exactly the planted corners."""
    p = synth.generate(synth.Config(**VI_CFG))
    planted = _plant_outliers(p)
    cal, orc, corners = _load_pair(p, calibrate_imu=True, max_iters=100, num_threads=8)
    want = _planted_mask(corners, planted)
    orc.solve()
    ro, fo, co = orc.residuals()
    mag_o = np.sqrt((ro ** 2).sum(axis=1))
    a = _view_order(corners["frame"], corners["camera"]); b = _view_order(fo, co)
    over = np.zeros(len(mag_o), dtype=bool); over[a] = mag_o[b] > 2.0 * orc.rmse()[0]
    print("oracle: camera RMSE %.3f px, planted |r| %.1f..%.1f px, largest other %.2f px" % (orc.rmse()[0], mag_o[b][want[a]].min(), mag_o[b][want[a]].max(), mag_o[b][~want[a]].max()))
    np.testing.assert_array_equal(over, want)
    cal.SetMaxIters(100); cal.SetRemoveOutliers(True, 2.0); cal.Solve()
    rep = cal.report()
    np.testing.assert_array_equal(rep["flags"] != 0, want)
    assert np.all(rep["flags"][want] == 2)                         # one copy fewer
    assert np.all(np.sqrt((rep["r"] ** 2).sum(axis=1))[want] > 20.0)
    _check_views(rep, cal)
    assert rep["views"]["removed"].sum() == 10 and rep["views"]["count"].sum() == len(want)


def test_a_model_misfit_shows_in_the_error_map():
    """Item 6: the share of the squared error that the map explains, sum_cells (sum_ru^2 + sum_rv^2) / count / sum |r|^2, from the report
    alone: about occupied cells / corners for noise, near 1 for a pattern.  kb4 pixels calibrated as kb4 and as `linear`."""
    p = synth.generate(synth.Config(models=("kb4",), n_frames=50, seed=11))
    assert p.n_obs == 9469

    def share(prob):
        cal = ViCalibrator(0).load_problem(prob); cal.SetCalibrateImu(False); cal.Solve()
        m = cal.report(bins=(16, 12))["maps"][0]
        occ = m[..., 0] > 0
        s = ((m[..., 1][occ] ** 2 + m[..., 2][occ] ** 2) / m[..., 0][occ]).sum() / m[..., 3].sum()
        print("occupied cells %d, share %.4f, camera RMSE %.3f px" % (occ.sum(), s, cal.GetCameraProjRMSE()[0]))
        return s, int(occ.sum())

    good, occ = share(p)
    assert occ == 105
    p.cam_model = [synth.MODEL_IDS["linear"]]; p.cam_K_init = [np.asarray(p.cam_K_init[0])[:4].copy()]; p.cam_K_gt = [np.asarray(p.cam_K_gt[0])[:4].copy()]
    bad, _ = share(p)
    assert good < 0.05 and bad > 0.3


def _cauchy_half(w):
    """1/2 rho(|w|^2) with ceres::CauchyLoss(100) as Ceres evaluates it: b = a^2, c = 1 / b, rho = b log(1 + s c) -- not log1p: for a
    small s the rounding of 1 + s c IS the value, and the pass's cost carries it."""
    s = (w * w).sum(axis=1)
    return 0.5 * 1e4 * np.log(1.0 + s * 1e-4)


def _imu_rows_against_oracle(cal, orc, rep, rot_only):
    """Whitened rows against the oracle's value with the product's weights, unwhitened rows with identity weights."""
    n = cal.NumFrames()
    W = cal.imu_weights()
    _oracle_takes_state(orc, cal, imu=True)
    orc.set_flags(True, True, rot_only, True)
    orc.prepare(vis_mult=1, imu_mult=1)
    orc.set_imu_weights(W)
    worst = 0.0
    for j in range(1, n):
        ro = orc.imu_value(j)
        tol = 1e-6 * max(np.abs(ro).max(), 1.0)
        worst = max(worst, np.abs(rep["imu"]["whitened"][j - 1] - ro).max() / tol)
        assert np.all(np.abs(rep["imu"]["whitened"][j - 1] - ro) <= tol)
    orc.set_imu_weights(np.tile(np.eye(9), (n - 1, 1, 1)))
    for j in range(1, n):
        ro = orc.imu_value(j)
        tol = 1e-6 * max(np.abs(ro).max(), 1.0)
        worst = max(worst, np.abs(rep["imu"]["unwhitened"][j - 1] - ro).max() / tol)
        assert np.all(np.abs(rep["imu"]["unwhitened"][j - 1] - ro) <= tol)
    print("IMU rows vs oracle: max of error / tolerance = %.3e" % worst)


@pytest.mark.parametrize("rot_only", [False, True])
def test_imu_blocks_against_the_oracle(rot_only):
    """Item 7: a held linearisation of the full inertial stage (or the rotation-only one) at a perturbed state; the report's rows against
    the oracle at identical parameters and weights, and 1/2 rho(|whitened|^2) against the block costs of the pass itself."""
    p = synth.generate(synth.Config(**VI_CFG))
    gt = p.imu_gt
    cal = ViCalibrator(0).load_problem(p, init=False)
    orc = ol.Oracle().load(p, init=False); orc.set_options(calibrate_imu=True)
    b0 = np.concatenate([gt["bg"], gt["ba"]]) * 0.8; s0 = np.concatenate([gt["sg"], gt["sa"]])
    cal.SetOptimizationFlags(True, True, rot_only, True)
    cal.SetBiases(b0); cal.SetScaleFactor(s0); cal.SetTimeOffset(0.002); cal.SetGravity(np.array([0.01, -0.02]))
    # twice: a pass linearises with the weights the pass before it left and then updates them from the accepted state; the second
    # held pass therefore linearises with the weights of THIS state, which are the current ones the report reads
    cal.linearize(); cal.linearize()
    _, _, cost = cal.imu_blocks()
    rep = cal.report()
    assert rep["imu"]["whitened"].shape == (59, 9) and not rep["imu"]["flags"].any()
    ref = _cauchy_half(rep["imu"]["whitened"])                      # imu_mult = 1: the pass's cost is multiplicity x rho, halved in the total
    rel = np.abs(0.5 * cost - ref) / np.maximum(ref, 1e-300)
    print("block cost vs 1/2 rho(|whitened|^2): max relative difference %.3e" % rel.max())
    assert np.all(np.abs(0.5 * cost - ref) <= 1e-12 * ref)
    if rot_only:
        assert not rep["imu"]["whitened"][:, [0, 1, 2, 6, 7, 8]].any() and not rep["imu"]["unwhitened"][:, [0, 1, 2, 6, 7, 8]].any()
        assert rep["imu"]["unwhitened"][:, 3:6].any()
    _imu_rows_against_oracle(cal, orc, rep, rot_only)
    _same_report(rep, cal.report())


def test_imu_blocks_after_the_full_schedule_and_with_a_truncated_stream():
    """Item 7: after the complete visual-inertial schedule (weights as the last pass left them), and test_gpu_parity's truncated IMU
    stream: the blocks past its end are flagged and zero."""
    p = synth.generate(synth.Config(**VI_CFG))
    cal = ViCalibrator(0).load_problem(p); cal.SetMaxIters(100); cal.Solve()
    rep = cal.report()
    orc = ol.Oracle().load(p); orc.set_options(calibrate_imu=True)
    _imu_rows_against_oracle(cal, orc, rep, False)
    _check_views(rep, cal)
    # truncated stream
    k = int(np.searchsorted(p.imu_t, p.frame_time[50]))
    cal = ViCalibrator(0)
    for c, m in enumerate(p.cam_model):
        cal.AddCamera(m, p.cam_K_gt[c], p.cam_T_ck_gt[c], p.cfg.width, p.cfg.height)
    for n in range(60):
        cal.AddFrame(p.frame_T_wk_gt[n], p.frame_time[n])
    for (f, c, ids, pix) in p.tiles:
        cal.AddObservations(f, c, p.grid_points[ids], pix)
    cal.AddImuMeasurements(p.imu_gyro[:k], p.imu_accel[:k], p.imu_t[:k])
    gt = p.imu_gt
    cal.SetOptimizationFlags(True, True, False, True); cal.SetBiases(np.concatenate([gt["bg"], gt["ba"]])); cal.SetScaleFactor(np.concatenate([gt["sg"], gt["sa"]]))
    cal.SetTimeOffset(0.002)
    cal.linearize(); cal.linearize()          # (twice: see test_imu_blocks_against_the_oracle)
    _, _, cost = cal.imu_blocks()
    rep = cal.report()
    fl = rep["imu"]["flags"]
    assert fl[49] == 0 and np.all(fl[50:] == 1) and not fl[:49].any()
    assert not rep["imu"]["whitened"][50:].any() and not rep["imu"]["unwhitened"][50:].any()
    ref = _cauchy_half(rep["imu"]["whitened"])
    assert np.all(np.abs(0.5 * cost - ref) <= 1e-12 * ref)


def test_a_report_moves_nothing():
    """Item 9: solve, report, Resume + solve gives the trace of the same sequence without the report; the pass keeps its forms."""
    p = synth.generate(synth.Config(**VI_CFG))
    traces, paths = [], []
    for with_report in (False, True):
        cal = ViCalibrator(0).load_problem(p); cal.SetMaxIters(100); cal.Solve()
        before = cal.pass_paths()
        if with_report:
            cal.report(); cal.report(bins=(7, 5))
        assert cal.pass_paths() == before
        cal.Resume(); cal.Solve()
        traces.append(cal.trace()); paths.append(cal.pass_paths())
    np.testing.assert_array_equal(traces[0], traces[1])
    assert paths[0] == paths[1]
    # ... and a report before the first solve does not change that solve either
    p = synth.generate(synth.BASELINE_CONFIGS["cfg1"])
    traces = []
    for with_report in (False, True):
        cal = ViCalibrator(0).load_problem(p); cal.SetCalibrateImu(False)
        if with_report:
            cal.report()
        cal.Solve(); traces.append(cal.trace())
    np.testing.assert_array_equal(traces[0], traces[1])


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close(); return port


def test_two_ranks_report_their_own_frames():
    """Item 8: two ranks on one GPU over gloo, no solve (tests/report_worker.py)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(HERE, "report_worker.py")]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", VICALIB_AMD_FLAG_SYNC="0")
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    fail = out.stdout.find("WORKER-FAILURE")
    assert out.returncode == 0, (out.stdout[fail:fail + 7000] if fail >= 0 else out.stdout[-3000:] + out.stderr[-3000:])
    assert out.stdout.count("ok") >= 2


# ------------------------------------------------------------------------------------------ command line
TOOL = os.path.join(os.path.dirname(HERE), "vicalib_amd", "vicalib")


def _masked(stdout):
    import re
    return [re.sub(r"solve time: [0-9.]+ s", "solve time: X s", ln) for ln in stdout.splitlines()]


def test_cli_report_files(tmp_path):
    """Item 10: -report_dir writes the files, views.csv's worst row is the planted view, corners.csv carries the library's residuals,
    -report_worst names the view; without a report flag the tool writes and prints what it did before."""
    p = synth.generate(synth.BASELINE_CONFIGS["cfg1"])
    f20, _ = _plant_noisy_view(p)
    data = tmp_path / "data"; os.makedirs(data)
    synth.write_dataset(p, str(data))
    base = [TOOL, "-cam", "detections://" + str(data / "cam0.csv"), "-models", "poly3", "-calibrate_imu=false", "-grid_preset", "small"]
    plain_dir = tmp_path / "plain"; rep_dir = tmp_path / "rep"; os.makedirs(plain_dir); os.makedirs(rep_dir)
    plain = subprocess.run(base + ["-output", "cameras.xml"], cwd=plain_dir, capture_output=True, text=True, timeout=600)
    withr = subprocess.run(base + ["-output", "cameras.xml", "-report_dir", "report", "-report_worst", "1"], cwd=rep_dir, capture_output=True, text=True, timeout=600)
    assert plain.returncode in (0, 2) and withr.returncode == plain.returncode, (plain.stderr[-2000:], withr.stderr[-2000:])
    assert sorted(os.listdir(plain_dir)) == ["cameras.xml"]
    assert sorted(os.listdir(rep_dir)) == ["cameras.xml", "report"]
    assert sorted(os.listdir(rep_dir / "report")) == ["corners.csv", "error_map_cam0.csv", "views.csv"]
    a, b = _masked(plain.stdout), _masked(withr.stdout)
    extra = [ln for ln in b if "worst views" in ln or ln.startswith("  frame ")]
    assert [ln for ln in b if ln not in extra] == a and len(extra) == 2
    assert extra[1].startswith("  frame %d:" % f20)
    views = np.genfromtxt(rep_dir / "report" / "views.csv", delimiter=",", names=True)
    assert len(views) == 50 and list(views.dtype.names) == ["frame", "camera", "corners", "removed", "rmse_px", "max_px", "worst_dot"]
    assert int(views["frame"][np.argmax(views["rmse_px"])]) == f20
    rows = np.genfromtxt(rep_dir / "report" / "corners.csv", delimiter=",", names=True)
    assert len(rows) == 8055 and list(rows.dtype.names) == ["frame", "camera", "dot", "u", "v", "ru", "rv", "removed"]
    cells = np.genfromtxt(rep_dir / "report" / "error_map_cam0.csv", delimiter=",", names=True)
    assert len(cells) == 16 * 12 and cells["count"].sum() == 8055
    # the library on the same detections, the tool's flow (start intrinsics of -models poly3, PnP seed, Start(has_initial_guess = false))
    cal = ViCalibrator(0)
    cal.AddCamera("poly3", [300, 300, p.cfg.width / 2.0, p.cfg.height / 2.0, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0], p.cfg.width, p.cfg.height)
    cal.SetBiases(np.zeros(6)); cal.SetScaleFactor(np.ones(6))
    for n in range(len(p.frame_time)):
        cal.AddFrame([0, 0, 0, 1, 0, 0, 1000], p.frame_time[n])
    for (f, c, ids, pix) in p.tiles:
        cal.AddObservations(f, c, p.grid_points[ids], pix)
    cal.SetPnPRansac(0, 2.0); cal.InitFramePosesPnP()
    cal.SetOptimizationFlags(False, False, True, True); cal.SetFunctionTolerance(1e-6); cal.SetMaxIters(200); cal.SetCalibrateImu(False)
    cal.Solve()
    rep = cal.report()
    csv = np.stack([rows["ru"], rows["rv"]], axis=1)
    # %.10g: ten significant digits
    assert np.all(np.abs(csv - rep["r"]) <= 1e-9 * np.abs(rep["r"]) + 1e-12)
    np.testing.assert_array_equal(rows["frame"].astype(int), rep["frame"])


def test_cli_report_files_visual_inertial(tmp_path):
    """Item 10 with the IMU: the fourth file, one row per IMU block."""
    p = synth.generate(synth.Config(**VI_CFG))
    files, imu_dir = synth.write_dataset(p, str(tmp_path / "data"))
    r = subprocess.run([TOOL, "-cam", "detections://" + files[0], "-imu", "csv://" + imu_dir, "-models", "kb4", "-grid_preset", "small", "-max_iters", "100",
                        "-report_dir", "report", "-report_bins", "8x6"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 2), r.stderr[-3000:]
    assert sorted(os.listdir(tmp_path / "report")) == ["corners.csv", "error_map_cam0.csv", "imu_blocks.csv", "views.csv"]
    blocks = np.genfromtxt(tmp_path / "report" / "imu_blocks.csv", delimiter=",", names=True)
    assert len(blocks) == 59 and len(blocks.dtype.names) == 21 and blocks.dtype.names[0] == "frame" and blocks.dtype.names[-1] == "flag"
    np.testing.assert_array_equal(blocks["frame"].astype(int), np.arange(59))
    assert len(np.genfromtxt(tmp_path / "report" / "error_map_cam0.csv", delimiter=",", names=True)) == 48
