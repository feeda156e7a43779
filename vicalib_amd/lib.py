"""ctypes binding of the C ABI (include/vicalib_amd.h) -- used by tests/ and bench.py.

`ViCalibrator` mirrors the public API of the reference class of the same name
(include/vicalib/vicalibrator.h:119-544): same method names and argument meaning, so the parity
tests read like code written against the reference.  There is no fallback: if the HIP library is
missing or no GPU is present, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VICALIB_AMD_LIB") or os.path.join(_HERE, "libvicalib_amd.so")
_lib = None

VC_OK = 0
ERRORS = {-1: "VC_ERR_NO_DEVICE", -2: "VC_ERR_BAD_ARG", -3: "VC_ERR_RUNNING", -4: "VC_ERR_TIME_ORDER",
          -5: "VC_ERR_TOO_MANY_POINTS", -6: "VC_ERR_NUMERIC", -7: "VC_ERR_UNSUPPORTED", -8: "VC_ERR_NO_CONVERGENCE"}
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int)

# every symbol include/vicalib_amd.h declares
SYMBOLS = [
    "vc_create", "vc_destroy", "vc_clear", "vc_add_camera", "vc_fix_camera_intrinsics", "vc_add_frame", "vc_set_frame_pose",
    "vc_add_observations", "vc_add_observation_tiles", "vc_add_imu", "vc_set_sigmas", "vc_set_biases", "vc_set_scale_factor", "vc_set_time_offset",
    "vc_set_function_tolerance", "vc_set_optimization_flags", "vc_set_max_iters", "vc_set_tolerances", "vc_set_gravity", "vc_set_frame_velocities", "vc_set_calibrate_imu", "vc_set_remove_outliers",
    "vc_solve", "vc_start", "vc_resume", "vc_set_stage_limit", "vc_sync_timeouts", "vc_set_kernel_timing", "vc_get_kernel_timing", "vc_is_running", "vc_stop", "vc_num_frames", "vc_num_imu_blocks", "vc_num_cameras", "vc_get_camera", "vc_get_frame",
    "vc_get_biases", "vc_get_scale_factor", "vc_get_gravity", "vc_time_offset", "vc_mean_squared_error", "vc_get_camera_proj_rmse",
    "vc_get_num_iterations", "vc_num_imu_measurements", "vc_get_imu_measurements", "vc_get_integration_poses", "vc_print_results", "vc_write_camera_models", "vc_trace_len", "vc_get_trace", "vc_set_shard", "vc_get_stream", "vc_prepare",
    "vc_linearize", "vc_step_hold", "vc_shared_dim", "vc_run_iterations", "vc_download_state", "vc_evaluate", "vc_time_kernels", "vc_time_stages", "vc_get_imu_blocks", "vc_get_debug_stamps", "vc_num_observations", "vc_num_tiles",
    "vc_init_frame_poses_pnp", "vc_pnp_planar", "vc_pnp_planar_ransac", "vc_set_pnp_ransac", "vc_pnp_planar_batch", "vc_time_pnp_planar_batch", "vc_set_pnp_device", "vc_seed_focal_batch", "vc_time_seed_focal_batch", "vc_dot_bias_batch", "vc_time_dot_bias_batch", "vc_rccl_unique_id", "vc_set_shard_rccl", "vc_shard_comm_create", "vc_set_shard_comm", "vc_shard_comm_destroy", "vc_allreduce_calls", "vc_shard_info", "vc_pass_paths", "vc_chain_order", "vc_last_error", "vc_get_imu_weights",
    "vc_solution_covariance_dim", "vc_get_solution_covariance", "vc_get_solution_covariance_names",
    "vc_target_make_pattern", "vc_target_find",
    "vc_report_compute", "vc_report_num_corners", "vc_report_corners", "vc_report_num_views", "vc_report_views", "vc_report_error_map", "vc_report_num_imu_blocks", "vc_report_imu", "vc_time_report_sweeps",
    "vc_holdout_clear", "vc_holdout_add_tiles", "vc_holdout_compute", "vc_holdout_num_frames", "vc_holdout_num_views", "vc_holdout_num_corners", "vc_holdout_frames", "vc_holdout_views",
    "vc_holdout_corners", "vc_holdout_camera_rmse", "vc_time_holdout",
    "vc_detector_create", "vc_detector_destroy", "vc_detector_set_params", "vc_detector_find", "vc_detector_find_conics",
    "vc_undistorter_create", "vc_undistorter_create_for_camera", "vc_undistorter_destroy", "vc_undistort_fit_linear", "vc_undistort_images",
    "vc_undistort_images_device", "vc_undistort_stream", "vc_undistort_points", "vc_undistort_get_map", "vc_undistort_get_linear", "vc_time_undistort",
    "vc_stereo_rectify_rotations", "vc_stereo_fit_linear", "vc_match_tiles", "vc_rectifier_create", "vc_rectifier_create_for_cameras", "vc_rectifier_destroy",
    "vc_rectifier_side", "vc_rectifier_get", "vc_rectify_pairs", "vc_rectify_check", "vc_time_rectify_check",
    "vc_comparer_create", "vc_comparer_create_for_camera", "vc_comparer_destroy", "vc_compare_run", "vc_compare_get_fit", "vc_compare_get_map",
    "vc_compare_summary", "vc_compare_rings", "vc_compare_extrinsics", "vc_time_compare",
    "vc_converter_create", "vc_converter_create_for_camera", "vc_converter_destroy", "vc_convert_run", "vc_convert_get", "vc_convert_comparer", "vc_time_convert",
    "vc_uncertainty_create", "vc_uncertainty_create_for_camera", "vc_uncertainty_destroy", "vc_uncertainty_run", "vc_uncertainty_get_fit", "vc_uncertainty_get_map",
    "vc_uncertainty_summary", "vc_uncertainty_rings", "vc_time_uncertainty",
    "vc_stereo_pose_jacobian", "vc_stereo_uncertainty_create", "vc_stereo_uncertainty_create_for_cameras", "vc_stereo_uncertainty_destroy", "vc_stereo_uncertainty_get",
    "vc_stereo_uncertainty_run", "vc_stereo_uncertainty_get_map", "vc_stereo_uncertainty_summary", "vc_stereo_uncertainty_get_pose_sigma", "vc_time_stereo_uncertainty",
    "vc_selector_create", "vc_selector_create_for_calibrator", "vc_selector_destroy", "vc_select_add_tiles", "vc_select_set_poses", "vc_select_run", "vc_select_get",
    "vc_select_frames", "vc_select_frame_information", "vc_select_last_gains", "vc_select_dim", "vc_time_select",
    "vc_registrar_create", "vc_registrar_create_for_cameras", "vc_registrar_destroy", "vc_register_get", "vc_register_depth", "vc_register_depth_device",
    "vc_register_stream", "vc_register_color", "vc_register_points", "vc_time_register",
    "vc_depthcal_create", "vc_depthcal_create_for_camera", "vc_depthcal_destroy", "vc_depthcal_get", "vc_depthcal_clear", "vc_depthcal_add", "vc_depthcal_expected",
    "vc_depthcal_sums", "vc_depthcal_fit", "vc_depthcal_get_fit", "vc_depthcal_set_fit", "vc_depthcal_apply", "vc_time_depthcal",
    "vc_allan_create", "vc_allan_destroy", "vc_allan_get", "vc_allan_static", "vc_allan_set_range", "vc_allan_run", "vc_time_allan", "vc_allan_factors", "vc_allan_fit",
    "vc_seed_imu_sweep", "vc_seed_imu", "vc_time_seed_imu",
    "vc_seed_rig", "vc_time_seed_rig",
    "vc_target_refine_batch", "vc_time_target_refine_batch",
]


class VicalibError(RuntimeError):
    pass


def target_make_pattern(rows, cols, seed=71):
    """vc_target_make_pattern: rows x cols array, 1 = large dot."""
    out = np.zeros((rows, cols), dtype=np.int32)
    _check(load().vc_target_make_pattern(int(rows), int(cols), C.c_uint(seed), out.ctypes.data_as(C.c_void_p)), "target_make_pattern")
    return out


def target_find(centres, conics, pattern):
    """vc_target_find: dot index (row * cols + col, or -1) of every conic; an all -1 result means no unambiguous placement."""
    centres = np.ascontiguousarray(centres, dtype=np.float64); conics = np.ascontiguousarray(conics, dtype=np.float64)
    pattern = np.ascontiguousarray(pattern, dtype=np.int32)
    n = len(centres)
    idx = np.full(n, -1, dtype=np.int32); m = C.c_int(0)
    _check(load().vc_target_find(_d(centres), _d(conics), n, pattern.ctypes.data_as(C.c_void_p), pattern.shape[0], pattern.shape[1],
                                 idx.ctypes.data_as(C.c_void_p), C.byref(m)), "target_find")
    return idx, m.value


def pnp_planar(model, params, p_w, p_c):
    """T_cw and RMS reprojection error (pixels) of one view of the planar grid (vc_pnp_planar; host code, needs no GPU)."""
    L = load()
    params = np.ascontiguousarray(params, dtype=np.float64)
    p_w = np.ascontiguousarray(p_w, dtype=np.float64); p_c = np.ascontiguousarray(p_c, dtype=np.float64)
    T = np.zeros(7); rms = C.c_double(0)
    from .synth import MODEL_IDS
    m = MODEL_IDS[model] if isinstance(model, str) else int(model)
    _check(L.vc_pnp_planar(m, _d(params), len(params), len(p_w), _d(p_w), _d(p_c), _d(T), C.byref(rms)), "pnp_planar")
    return T, rms.value


def pnp_planar_ransac(model, params, p_w, p_c, iterations=64, tol_px=2.0):
    """Robust pose of one view (vc_pnp_planar_ransac): T_cw, RMS over the inliers, inlier flags."""
    L = load()
    params = np.ascontiguousarray(params, dtype=np.float64)
    p_w = np.ascontiguousarray(p_w, dtype=np.float64); p_c = np.ascontiguousarray(p_c, dtype=np.float64)
    T = np.zeros(7); rms = C.c_double(0); n_in = C.c_int(0); flags = np.zeros(len(p_w), dtype=np.int8)
    from .synth import MODEL_IDS
    m = MODEL_IDS[model] if isinstance(model, str) else int(model)
    _check(L.vc_pnp_planar_ransac(m, _d(params), len(params), len(p_w), _d(p_w), _d(p_c), int(iterations), C.c_double(tol_px), _d(T),
                                  C.byref(rms), C.byref(n_in), flags.ctypes.data_as(C.c_void_p)), "pnp_planar_ransac")
    return T, rms.value, flags.astype(bool)


def _pnp_batch_arrays(models, params, view_off, p_w, p_c):
    from .synth import MODEL_IDS
    n = len(models)
    m = np.array([MODEL_IDS[x] if isinstance(x, str) else int(x) for x in models], dtype=np.int32)
    K = np.zeros((n, 10))
    for v in range(n):
        K[v, :len(params[v])] = params[v]
    off = np.ascontiguousarray(view_off, dtype=np.int32)
    p_w = np.ascontiguousarray(p_w, dtype=np.float64).reshape(-1, 3); p_c = np.ascontiguousarray(p_c, dtype=np.float64).reshape(-1, 2)
    return n, m, K, off, p_w, p_c


def time_pnp_planar_batch(models, params, view_off, p_w, p_c, iterations=0, tol_px=0.0, device=0, reps=10):
    """mean time in ms of the kernel of pnp_planar_batch alone on that input (vc_time_pnp_planar_batch: HIP events, launches back to back)"""
    n, m, K, off, p_w, p_c = _pnp_batch_arrays(models, params, view_off, p_w, p_c)
    ms = C.c_double(0)
    _check(load().vc_time_pnp_planar_batch(int(device), n, m.ctypes.data_as(C.c_void_p), _d(K), off.ctypes.data_as(C.c_void_p), _d(p_w), _d(p_c), int(iterations),
                                           C.c_double(tol_px), int(reps), C.byref(ms)), "time_pnp_planar_batch")
    return ms.value


def pnp_planar_batch(models, params, view_off, p_w, p_c, iterations=0, tol_px=0.0, device=0, out=None):
    """Poses of many views at once on the device (vc_pnp_planar_batch).  models: per view (names or ids); params: per view, up to 10 each;
    view v owns corners view_off[v] .. view_off[v+1]-1 of p_w / p_c.  Returns T_cw [n, 7], rms, n_inliers, inlier (bool per corner), status;
    `out` may hold pre-filled T_cw / rms / n_inliers arrays: a view with status != 0 leaves its rows as they were."""
    L = load()
    n, m, K, off, p_w, p_c = _pnp_batch_arrays(models, params, view_off, p_w, p_c)
    out = dict(out or {})
    T = out.get("T_cw", np.zeros((n, 7))); rms = out.get("rms", np.zeros(n)); n_in = out.get("n_inliers", np.zeros(n, dtype=np.int32))
    assert T.dtype == np.float64 and rms.dtype == np.float64 and n_in.dtype == np.int32 and T.flags.c_contiguous
    flags = np.zeros(max(len(p_w), 1), dtype=np.int8); status = np.full(max(n, 1), -1, dtype=np.int32)
    pad3, pad2 = (p_w if len(p_w) else np.zeros((1, 3))), (p_c if len(p_c) else np.zeros((1, 2)))
    _check(L.vc_pnp_planar_batch(int(device), n, m.ctypes.data_as(C.c_void_p), _d(K), off.ctypes.data_as(C.c_void_p), _d(pad3), _d(pad2), int(iterations),
                                 C.c_double(tol_px), T.ctypes.data_as(C.c_void_p), rms.ctypes.data_as(C.c_void_p), n_in.ctypes.data_as(C.c_void_p),
                                 flags.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)), "pnp_planar_batch")
    return dict(T_cw=T, rms=rms, n_inliers=n_in, inlier=flags[:len(p_w)].astype(bool), status=status[:n])


def _focal_batch_arrays(view_cam, cam_pp, cam_radius, view_off, p_w, p_c):
    cam = np.ascontiguousarray(view_cam, dtype=np.int32).reshape(-1)
    pp = np.ascontiguousarray(cam_pp, dtype=np.float64).reshape(-1, 2)
    rad = np.ascontiguousarray(cam_radius, dtype=np.float64).reshape(-1)
    off = np.ascontiguousarray(view_off, dtype=np.int32).reshape(-1)
    p_w = np.ascontiguousarray(p_w, dtype=np.float64).reshape(-1, 3); p_c = np.ascontiguousarray(p_c, dtype=np.float64).reshape(-1, 2)
    if len(off) != len(cam) + 1 or len(rad) != len(pp):
        raise VicalibError("seed_focal_batch: view_off needs one entry more than view_cam, cam_radius one per row of cam_pp")
    pad = lambda a, shape, dt: a if len(a) else np.zeros(shape, dtype=dt)
    return cam, pp, rad, off, pad(p_w, (1, 3), np.float64), pad(p_c, (1, 2), np.float64), pad(cam, 1, np.int32)


def seed_focal_batch(view_cam, cam_pp, cam_radius, view_off, p_w, p_c, min_corners=4, max_fit_px=0.0, min_tilt_deg=5.0, device=0, out=None):
    """The focal length of every camera from its views of the planar target, on the device (vc_seed_focal_batch).  view_cam: the camera of
    every view; cam_pp [n_cams, 2]: the assumed principal points; cam_radius [n_cams]: the corners used lie within that many pixels of it
    (<= 0: all); view v owns corners view_off[v] .. view_off[v+1]-1 of p_w / p_c.  Returns view_H [n, 3, 3], view_rows [n, 4] (c1 d1 c2 d2),
    view_f, view_fit_px, view_used, view_status, cam_f, cam_views, cam_status.  `out` may hold pre-filled view_H / view_rows / view_f /
    view_fit_px / view_used / cam_f arrays: a refused view or camera leaves its rows as they were (the default fill is NaN, 0 for view_used)."""
    L = load()
    cam, pp, rad, off, p_w, p_c, cam_arg = _focal_batch_arrays(view_cam, cam_pp, cam_radius, view_off, p_w, p_c)
    n, nc = len(cam), len(rad)
    out = dict(out or {})
    H = out.get("view_H", np.full((n, 3, 3), np.nan)); rows = out.get("view_rows", np.full((n, 4), np.nan)); f = out.get("view_f", np.full(n, np.nan))
    fit = out.get("view_fit_px", np.full(n, np.nan)); used = out.get("view_used", np.zeros(n, dtype=np.int32)); cam_f = out.get("cam_f", np.full(nc, np.nan))
    for a in (H, rows, f, fit, cam_f):
        assert a.dtype == np.float64 and a.flags.c_contiguous
    assert used.dtype == np.int32
    status = np.full(max(n, 1), -1, dtype=np.int32); cam_views = np.zeros(max(nc, 1), dtype=np.int32); cam_status = np.full(max(nc, 1), -1, dtype=np.int32)
    keep = [np.zeros(1) if a.size == 0 else a for a in (H, rows, f, fit, cam_f)] + [np.zeros(1, dtype=np.int32) if used.size == 0 else used]
    ip = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(L.vc_seed_focal_batch(int(device), n, ip(cam_arg), nc, _d(pp), _d(rad), ip(off), _d(p_w), _d(p_c), int(min_corners), C.c_double(max_fit_px),
                                 C.c_double(min_tilt_deg), _d(keep[0]), _d(keep[1]), _d(keep[2]), _d(keep[3]), ip(keep[5]), ip(status), _d(keep[4]), ip(cam_views),
                                 ip(cam_status)), "seed_focal_batch")
    return dict(view_H=H, view_rows=rows, view_f=f, view_fit_px=fit, view_used=used, view_status=status[:n], cam_f=cam_f, cam_views=cam_views[:nc],
                cam_status=cam_status[:nc])


def time_seed_focal_batch(view_cam, cam_pp, cam_radius, view_off, p_w, p_c, min_corners=4, max_fit_px=0.0, min_tilt_deg=5.0, device=0, reps=10):
    """mean time in ms of the two kernels of seed_focal_batch alone on that input (vc_time_seed_focal_batch: HIP events, runs back to back)"""
    cam, pp, rad, off, p_w, p_c, cam_arg = _focal_batch_arrays(view_cam, cam_pp, cam_radius, view_off, p_w, p_c)
    ms = C.c_double(0)
    ip = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(load().vc_time_seed_focal_batch(int(device), len(cam), ip(cam_arg), len(rad), _d(pp), _d(rad), ip(off), _d(p_w), _d(p_c), int(min_corners),
                                           C.c_double(max_fit_px), C.c_double(min_tilt_deg), int(reps), C.byref(ms)), "time_seed_focal_batch")
    return ms.value


def _dot_bias_arrays(models, params, T_cw, view_off, p_w, radius):
    from .synth import MODEL_IDS
    n = len(models)
    m = np.array([MODEL_IDS[x] if isinstance(x, str) else int(x) for x in models], dtype=np.int32)
    K = np.zeros((n, 10))
    for v in range(n):
        K[v, :len(params[v])] = params[v]
    T = np.ascontiguousarray(T_cw, dtype=np.float64).reshape(-1, 7)
    off = np.ascontiguousarray(view_off, dtype=np.int32).reshape(-1)
    p_w = np.ascontiguousarray(p_w, dtype=np.float64).reshape(-1, 3); rad = np.ascontiguousarray(radius, dtype=np.float64).reshape(-1)
    if len(T) != n or len(off) != n + 1 or len(rad) != len(p_w) or off[0] != 0 or off[-1] != len(rad):
        raise VicalibError("dot_bias_batch: T_cw needs one row per view, view_off one entry more from 0 to the number of observations, radius one per row of p_w")
    pad = lambda a, shape, dt: a if len(a) else np.zeros(shape, dtype=dt)
    return n, pad(m, 1, np.int32), pad(K, (1, 10), np.float64), pad(T, (1, 7), np.float64), off, pad(p_w, (1, 3), np.float64), pad(rad, 1, np.float64), len(rad)


def dot_bias_batch(models, params, T_cw, view_off, p_w, radius, device=0, out=None):
    """The predicted bias of every dot's measured centre, on the device (vc_dot_bias_batch).  models / params / T_cw: per view (names or ids; up to
    10 parameters each; target into camera [qx qy qz qw tx ty tz]); view v owns observations view_off[v] .. view_off[v+1]-1 of p_w [n, 3] (dot
    centres on the target) and radius [n] (metres).  Returns bias [n, 2] (pixels: subtract it from a measured centre), radius_px [n], status [n];
    `out` may hold pre-filled bias / radius_px arrays: an observation with status != 0 leaves its rows as they were (the default fill is NaN)."""
    nv, m, K, T, off, p_w, rad, n = _dot_bias_arrays(models, params, T_cw, view_off, p_w, radius)
    out = dict(out or {})
    bias = out.get("bias", np.full((n, 2), np.nan)); rpx = out.get("radius_px", np.full(n, np.nan))
    for a in (bias, rpx):
        assert a.dtype == np.float64 and a.flags.c_contiguous
    status = np.full(max(n, 1), -1, dtype=np.int32)
    keep = [np.zeros(2) if bias.size == 0 else bias, np.zeros(1) if rpx.size == 0 else rpx]
    ip = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(load().vc_dot_bias_batch(int(device), nv, ip(m), _d(K), _d(T), ip(off), _d(p_w), _d(rad), _d(keep[0]), _d(keep[1]), ip(status)), "dot_bias_batch")
    return dict(bias=bias, radius_px=rpx, status=status[:n])


def time_dot_bias_batch(models, params, T_cw, view_off, p_w, radius, device=0, reps=10):
    """mean time in ms of the kernel of dot_bias_batch alone on that input (vc_time_dot_bias_batch: HIP events, launches back to back)"""
    nv, m, K, T, off, p_w, rad, n = _dot_bias_arrays(models, params, T_cw, view_off, p_w, radius)
    ms = C.c_double(0)
    ip = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(load().vc_time_dot_bias_batch(int(device), nv, ip(m), _d(K), _d(T), ip(off), _d(p_w), _d(rad), int(reps), C.byref(ms)), "time_dot_bias_batch")
    return ms.value


def _target_refine_arrays(cameras, poses, tile_frame, tile_cam, tile_off, point_id, p_c, points, nominal):
    from .synth import MODEL_IDS
    n = len(cameras)
    model = np.array([MODEL_IDS[c[0]] if isinstance(c[0], str) else int(c[0]) for c in cameras], dtype=np.int32)
    params = np.zeros((max(n, 1), 10))
    for i, c in enumerate(cameras):
        params[i, :len(c[1])] = c[1]
    T_ck = np.ascontiguousarray([c[2] for c in cameras], dtype=np.float64).reshape(-1, 7)
    flags = np.array([c[3] for c in cameras], dtype=np.int32)
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
    tf = np.ascontiguousarray(tile_frame, dtype=np.int32).reshape(-1); tc = np.ascontiguousarray(tile_cam, dtype=np.int32).reshape(-1)
    off = np.ascontiguousarray(tile_off, dtype=np.int64).reshape(-1)
    pid = np.ascontiguousarray(point_id, dtype=np.int32).reshape(-1); z = np.ascontiguousarray(p_c, dtype=np.float64).reshape(-1, 2)
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3); nominal = np.ascontiguousarray(nominal, dtype=np.float64).reshape(-1, 3)
    if len(off) != len(tf) + 1 or len(tc) != len(tf) or len(z) != len(pid) or len(points) != len(nominal) or (len(off) and off[-1] > len(pid)):
        raise VicalibError("target_refine_batch: tile_off needs one entry more than tile_frame / tile_cam and ends within point_id, p_c one row per point_id, "
                           "nominal one row per row of points")
    pad = lambda a, shape, dt: a if len(a) else np.zeros(shape, dtype=dt)
    return (n, pad(model, 1, np.int32), params, pad(T_ck, (1, 7), np.float64), pad(flags, 1, np.int32), len(poses), pad(poses, (1, 7), np.float64), len(tf),
            pad(tf, 1, np.int32), pad(tc, 1, np.int32), off, pad(pid, 1, np.int32), pad(z, (1, 2), np.float64), pad(points, (1, 3), np.float64),
            pad(nominal, (1, 3), np.float64), len(points))


def target_refine_batch(cameras, poses, tile_frame, tile_cam, tile_off, point_id, p_c, points, nominal, lam, device=0, out=None):
    """One Gauss-Newton step on the target's points, the frame poses and the shared camera columns marginalised, on the device
    (vc_target_refine_batch).  cameras: [(model, K, T_ck, flags)] as for Selector; poses [N, 7]; tile t holds corners tile_off[t] .. tile_off[t+1]-1 of
    point_id / p_c (measured pixels) of (tile_frame[t], tile_cam[t]); points / nominal [P, 3]; lam: the prior's weight 1 / sigma^2.  Returns refined
    [P, 3], point_status, point_corners, frame_status, corners, behind (per frame), gauge_rank, result_status (0 ok, 1 singular), cost,
    predicted_decrease.  `out` may hold a pre-filled refined array: a singular result leaves it, cost and predicted_decrease (NaN) as they were."""
    a = _target_refine_arrays(cameras, poses, tile_frame, tile_cam, tile_off, point_id, p_c, points, nominal)
    N, P = a[5], a[15]
    out = dict(out or {})
    refined = out.get("refined", np.full((max(P, 1), 3), np.nan))
    assert refined.dtype == np.float64 and refined.flags.c_contiguous and refined.size >= 3 * P
    pstat = np.full(max(P, 1), -1, dtype=np.int32); pcor = np.zeros(max(P, 1), dtype=np.int32); fstat = np.zeros((max(N, 1), 3), dtype=np.int32)
    rank, status = C.c_int(0), C.c_int(-1)
    cost, pred = C.c_double(np.nan), C.c_double(np.nan)
    ip = lambda x: x.ctypes.data_as(C.c_void_p)
    _check(load().vc_target_refine_batch(int(device), a[0], ip(a[1]), _d(a[2]), _d(a[3]), ip(a[4]), N, _d(a[6]), a[7], ip(a[8]), ip(a[9]), ip(a[10]), ip(a[11]), _d(a[12]),
                                         _d(a[13]), _d(a[14]), P, C.c_double(lam), _d(refined), ip(pstat), ip(pcor), ip(fstat), C.byref(rank), C.byref(status),
                                         C.byref(cost), C.byref(pred)), "target_refine_batch")
    return dict(refined=refined[:P], point_status=pstat[:P], point_corners=pcor[:P], frame_status=fstat[:N, 0].copy(), corners=fstat[:N, 1].copy(),
                behind=fstat[:N, 2].copy(), gauge_rank=rank.value, result_status=status.value, cost=cost.value, predicted_decrease=pred.value)


TARGET_REFINE_STAGES = ("sweep", "assembly", "shared", "gauge", "factor", "solve")


def time_target_refine_batch(cameras, poses, tile_frame, tile_cam, tile_off, point_id, p_c, points, nominal, lam, device=0, reps=10):
    """mean time in ms of the six stages of target_refine_batch alone on that input (vc_time_target_refine_batch: HIP events between the stages)"""
    a = _target_refine_arrays(cameras, poses, tile_frame, tile_cam, tile_off, point_id, p_c, points, nominal)
    ms = np.zeros(6)
    ip = lambda x: x.ctypes.data_as(C.c_void_p)
    _check(load().vc_time_target_refine_batch(int(device), a[0], ip(a[1]), _d(a[2]), _d(a[3]), ip(a[4]), a[5], _d(a[6]), a[7], ip(a[8]), ip(a[9]), ip(a[10]), ip(a[11]),
                                              _d(a[12]), _d(a[13]), _d(a[14]), a[15], C.c_double(lam), int(reps), _d(ms)), "time_target_refine_batch")
    return dict(zip(TARGET_REFINE_STAGES, ms.tolist()))


def _seed_imu_arrays(frame_t, frame_q_wc, frame_ok, imu_t, gyro, accel):
    ft = np.ascontiguousarray(frame_t, dtype=np.float64).reshape(-1)
    fq = np.ascontiguousarray(frame_q_wc, dtype=np.float64)
    ok = np.ascontiguousarray(np.asarray(frame_ok) != 0, dtype=np.uint8).reshape(-1)
    it = np.ascontiguousarray(imu_t, dtype=np.float64).reshape(-1)
    g = np.ascontiguousarray(gyro, dtype=np.float64); a = np.ascontiguousarray(accel, dtype=np.float64)
    if fq.shape != (len(ft), 4) or len(ok) != len(ft) or g.shape != (len(it), 3) or a.shape != (len(it), 3):
        raise VicalibError("seed_imu: frame_q_wc needs the shape [n_frames, 4], frame_ok the length n_frames, gyro and accel the shape [n_samples, 3]")
    return ft, fq, ok, it, g, a


def seed_imu_sweep(frame_t, frame_q_wc, frame_ok, imu_t, gyro, accel, lags, max_gap_s=0.5, min_intervals=10, device=0):
    """The fit of the camera rates to the gyro rates at every lag, on the device (vc_seed_imu_sweep).  frame_q_wc: [x y z w] of R_wc per frame
    (frame_ok = 0: none); returns J [n_lags], R [n_lags, 3, 3], bias [n_lags, 3], count [n_lags], moments [n_lags, 18]."""
    ft, fq, ok, it, g, a = _seed_imu_arrays(frame_t, frame_q_wc, frame_ok, imu_t, gyro, accel)
    lags = np.ascontiguousarray(lags, dtype=np.float64).reshape(-1)
    n = len(lags)
    J = np.zeros(max(n, 1)); R = np.zeros((max(n, 1), 3, 3)); bias = np.zeros((max(n, 1), 3)); count = np.zeros(max(n, 1), dtype=np.int32); mom = np.zeros((max(n, 1), 18))
    ip = lambda x: x.ctypes.data_as(C.c_void_p)
    _check(load().vc_seed_imu_sweep(int(device), len(ft), _d(ft), _d(fq), ip(ok), len(it), _d(it), _d(g), _d(a), C.c_double(max_gap_s), int(min_intervals), n,
                                    _d(lags) if n else None, _d(J), _d(R), _d(bias), ip(count), _d(mom)), "seed_imu_sweep")
    return dict(J=J[:n], R=R[:n], bias=bias[:n], count=count[:n], moments=mom[:n])


def seed_imu(frame_t, frame_q_wc, frame_ok, imu_t, gyro, accel, range_s=0.5, step_s=0.0, fine=8, max_gap_s=0.5, min_intervals=10, device=0):
    """The inertial seed (vc_seed_imu): status (0 ok, 1 too few intervals, 2 the minimum on the edge of the range, 3 not finite), the coarse
    curve (coarse_lags, coarse_J) and, with status 0, time_offset, R_ck [3, 3], gyro_bias, g_dir, rms, signal, count."""
    ft, fq, ok, it, g, a = _seed_imu_arrays(frame_t, frame_q_wc, frame_ok, imu_t, gyro, accel)
    L = load()
    ip = lambda x: x.ctypes.data_as(C.c_void_p)
    off = C.c_double(0); rms = C.c_double(0); sig = C.c_double(0); count = C.c_int(0); status = C.c_int(-1); n_coarse = C.c_int(0)
    R = np.zeros((3, 3)); bias = np.zeros(3); g_dir = np.zeros(2)
    cap = 0
    for _ in range(2):                    # the coarse curve is caller-sized: the first call reports its length, a second one fetches a longer curve
        lags = np.zeros(max(cap, 4096)); J = np.zeros(max(cap, 4096))
        _check(L.vc_seed_imu(int(device), len(ft), _d(ft), _d(fq), ip(ok), len(it), _d(it), _d(g), _d(a), C.c_double(max_gap_s), int(min_intervals),
                             C.c_double(range_s), C.c_double(step_s), int(fine), C.byref(off), _d(R), _d(bias), _d(g_dir), C.byref(rms), C.byref(sig),
                             C.byref(count), C.byref(status), len(lags), _d(lags), _d(J), C.byref(n_coarse)), "seed_imu")
        if n_coarse.value <= len(lags):
            break
        cap = n_coarse.value
    out = dict(status=status.value, coarse_lags=lags[:n_coarse.value].copy(), coarse_J=J[:n_coarse.value].copy())
    if status.value == 0:
        out.update(time_offset=off.value, R_ck=R, gyro_bias=bias, g_dir=g_dir, rms=rms.value, signal=sig.value, count=count.value)
    return out


def time_seed_imu(frame_t, frame_q_wc, frame_ok, imu_t, gyro, accel, lags, max_gap_s=0.5, min_intervals=10, device=0, reps=10):
    """mean kernel times in ms (vc_time_seed_imu: HIP events, launches back to back): prepare (prefix integrals, camera rates), sweep, gravity"""
    ft, fq, ok, it, g, a = _seed_imu_arrays(frame_t, frame_q_wc, frame_ok, imu_t, gyro, accel)
    lags = np.ascontiguousarray(lags, dtype=np.float64).reshape(-1)
    ms = np.zeros(3)
    _check(load().vc_time_seed_imu(int(device), len(ft), _d(ft), _d(fq), ok.ctypes.data_as(C.c_void_p), len(it), _d(it), _d(g), _d(a), C.c_double(max_gap_s),
                                   int(min_intervals), len(lags), _d(lags), int(reps), _d(ms)), "time_seed_imu")
    return dict(prepare=ms[0], sweep=ms[1], gravity=ms[2])


def _seed_rig_arrays(view_ok, view_T_cw):
    ok = np.ascontiguousarray(np.asarray(view_ok) != 0, dtype=np.uint8)
    T = np.ascontiguousarray(view_T_cw, dtype=np.float64)
    if ok.ndim != 2 or ok.shape[1] < 1 or T.shape != ok.shape + (7,):
        raise VicalibError("seed_rig: view_ok needs the shape [n_frames, n_cams] with at least one camera, view_T_cw the shape [n_frames, n_cams, 7]")
    pad = lambda a, shape, dt: a if a.size else np.zeros(shape, dtype=dt)
    return ok.shape[0], ok.shape[1], pad(ok, 1, np.uint8), pad(T, 7, np.float64)


def seed_rig(view_ok, view_T_cw, tol_deg=3.0, min_support=3, device=0, out=None):
    """Every camera's pose relative to camera 0 from the views it shares, on the device (vc_seed_rig).  view_ok [n_frames, n_cams];
    view_T_cw [n_frames, n_cams, 7]: target into camera, [qx qy qz qw tx ty tz]; a view that is not ok is never read.  Returns, per pair (a < b)
    in the order (0,1), (0,2) .. (1,2) ..: pair_T_ab [n_pairs, 7] (camera b into camera a), pair_shared, pair_support, pair_winner, pair_rms_deg,
    pair_rms_m, pair_status (0 ok, 1 no shared frame, 2 support below min_support); per camera: cam_T_c0 [n_cams, 7] (camera 0 into camera c),
    cam_parent, cam_status (0 reached, 1 not connected).  `out` may hold pre-filled arrays of those names: a refused pair or a camera not
    reached leaves its rows as they were (the default fill is NaN, -1 for the counts)."""
    nf, nc, ok, T = _seed_rig_arrays(view_ok, view_T_cw)
    n_pairs = nc * (nc - 1) // 2
    out = dict(out or {})
    f64 = lambda k, shape: out.get(k, np.full(shape, np.nan))
    i32 = lambda k, n: out.get(k, np.full(n, -1, dtype=np.int32))
    r = dict(pair_T_ab=f64("pair_T_ab", (n_pairs, 7)), pair_shared=i32("pair_shared", n_pairs), pair_support=i32("pair_support", n_pairs),
             pair_winner=i32("pair_winner", n_pairs), pair_rms_deg=f64("pair_rms_deg", n_pairs), pair_rms_m=f64("pair_rms_m", n_pairs),
             pair_status=i32("pair_status", n_pairs), cam_T_c0=f64("cam_T_c0", (nc, 7)), cam_parent=i32("cam_parent", nc), cam_status=i32("cam_status", nc))
    for k, a in r.items():
        assert a.flags.c_contiguous and a.dtype == (np.float64 if k in ("pair_T_ab", "pair_rms_deg", "pair_rms_m", "cam_T_c0") else np.int32), k
    ip = lambda a: (a if a.size else np.zeros(1, dtype=a.dtype)).ctypes.data_as(C.c_void_p)
    _check(load().vc_seed_rig(int(device), nf, nc, ip(ok), ip(T), C.c_double(tol_deg), int(min_support), ip(r["pair_T_ab"]), ip(r["pair_shared"]),
                              ip(r["pair_support"]), ip(r["pair_winner"]), ip(r["pair_rms_deg"]), ip(r["pair_rms_m"]), ip(r["pair_status"]), ip(r["cam_T_c0"]),
                              ip(r["cam_parent"]), ip(r["cam_status"])), "seed_rig")
    return r


def time_seed_rig(view_ok, view_T_cw, tol_deg=3.0, min_support=3, device=0, reps=10):
    """mean kernel times in ms (vc_time_seed_rig: HIP events, launches back to back): candidates, support (the quadratic vote), finish, total"""
    nf, nc, ok, T = _seed_rig_arrays(view_ok, view_T_cw)
    ms = np.zeros(3)
    _check(load().vc_time_seed_rig(int(device), nf, nc, ok.ctypes.data_as(C.c_void_p), _d(T), C.c_double(tol_deg), int(min_support), int(reps), _d(ms)), "time_seed_rig")
    return dict(candidates=ms[0], support=ms[1], finish=ms[2], total=float(ms.sum()))


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VicalibError(f"{LIB_PATH} is missing: build it with vicalib_amd/csrc/build.sh (no CPU fallback exists)")
        L = C.CDLL(LIB_PATH)
        L.vc_time_offset.restype = C.c_double
        L.vc_mean_squared_error.restype = C.c_double
        L.vc_get_num_iterations.restype = C.c_uint
        L.vc_get_stream.restype = C.c_void_p
        L.vc_undistort_stream.restype = C.c_void_p
        L.vc_rectifier_side.restype = C.c_void_p
        L.vc_register_stream.restype = C.c_void_p
        L.vc_num_observations.restype = C.c_longlong
        L.vc_report_num_corners.restype = C.c_longlong
        L.vc_holdout_num_corners.restype = C.c_longlong
        L.vc_allreduce_calls.restype = C.c_longlong
        L.vc_last_error.restype = C.c_char_p
        for name in ("vc_destroy", "vc_detector_destroy", "vc_shard_comm_destroy", "vc_undistorter_destroy", "vc_rectifier_destroy", "vc_comparer_destroy", "vc_converter_destroy",
                     "vc_uncertainty_destroy", "vc_stereo_uncertainty_destroy", "vc_selector_destroy", "vc_registrar_destroy", "vc_depthcal_destroy", "vc_allan_destroy"):
            getattr(L, name).restype = None
        _lib = L
    return _lib


def _check(rc, what):
    if rc < 0:
        raise VicalibError(f"{what} failed: {ERRORS.get(rc, rc)}")
    return rc


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.c_void_p)


class ShardComm:
    """One RCCL communicator for all calibrators of this process (vc_shard_comm_create): created once -- collective, the 128-byte id
    travels through torch.distributed --, lent to calibrators with ViCalibrator.set_shard_comm, destroyed with close() after them."""

    def __init__(self, device, rank, world, group=None):
        import torch.distributed as dist
        self.L = load()
        self.rank, self.world = int(rank), int(world)
        buf = C.create_string_buffer(128)
        if rank == 0:
            _check(self.L.vc_rccl_unique_id(buf), "rccl_unique_id")
        box = [bytes(buf.raw)]
        if world > 1:
            dist.broadcast_object_list(box, src=0, group=group)
        self.h = C.c_void_p()
        rc = self.L.vc_shard_comm_create(int(device), self.rank, self.world, C.create_string_buffer(box[0], 128), C.byref(self.h))
        if rc != 0:
            self.h = None
            raise VicalibError("shard_comm_create: status %d: %s" % (rc, (self.L.vc_last_error() or b"").decode(errors="replace")))

    def close(self):
        if getattr(self, "h", None):
            self.L.vc_shard_comm_destroy(self.h)
            self.h = None


class ViCalibrator:
    def __init__(self, device: int = 0):
        self.L = load()
        self.h = C.c_void_p()
        _check(self.L.vc_create(C.byref(self.h), int(device)), "vc_create")
        self._cb = None
        self.nk = []

    def close(self):
        if getattr(self, "h", None):
            self.L.vc_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    # ---- reference API ---------------------------------------------------------------------
    def AddCamera(self, model, params, T_ck, width=640, height=480):
        params = np.ascontiguousarray(params, dtype=np.float64)
        self.nk.append(len(params))
        if isinstance(model, str):               # the -models strings of vicalib-engine.cc:203-253
            from .synth import MODEL_IDS
            model = MODEL_IDS[model]
        return _check(self.L.vc_add_camera(self.h, int(model), _d(params), len(params), int(width), int(height), _d(T_ck)), "AddCamera")

    def Clear(self):
        _check(self.L.vc_clear(self.h), "Clear")
        self.nk = []

    def FixCameraIntrinsics(self, should_fix=True):
        _check(self.L.vc_fix_camera_intrinsics(self.h, int(should_fix)), "FixCameraIntrinsics")

    def AddFrame(self, T_wk, time):
        return _check(self.L.vc_add_frame(self.h, _d(T_wk), C.c_double(time)), "AddFrame")

    def SetFramePose(self, frame, T_wk):
        _check(self.L.vc_set_frame_pose(self.h, int(frame), _d(T_wk)), "SetFramePose")

    def InitFramePosesPnP(self):
        """calibu::PosePnPRansac + the pose write of vicalib-task.cc:335-348; returns the number of frames initialised."""
        n = C.c_int(0)
        _check(self.L.vc_init_frame_poses_pnp(self.h, C.byref(n)), "InitFramePosesPnP")
        return n.value

    def SetPnPRansac(self, iterations, tol_px): _check(self.L.vc_set_pnp_ransac(self.h, int(iterations), C.c_double(tol_px)), "SetPnPRansac")

    def SetPnPDevice(self, on):
        """the seeds of InitFramePosesPnP and of HoldoutCompute(None) from the batched device PnP (vc_set_pnp_device); default off: the host routine"""
        _check(self.L.vc_set_pnp_device(self.h, int(bool(on))), "SetPnPDevice")

    def AddObservations(self, frame, camera, p_w, p_c):
        p_w = np.ascontiguousarray(p_w, dtype=np.float64); p_c = np.ascontiguousarray(p_c, dtype=np.float64)
        _check(self.L.vc_add_observations(self.h, int(frame), int(camera), int(len(p_w)), _d(p_w), _d(p_c)), "AddObservation")

    def AddObservationTiles(self, tile_frame, tile_cam, tile_off, points, point_id, p_c):
        """AddObservation over many (frame, camera) groups in one call (vc_add_observation_tiles)."""
        tf = np.ascontiguousarray(tile_frame, dtype=np.int32); tc = np.ascontiguousarray(tile_cam, dtype=np.int32)
        off = np.ascontiguousarray(tile_off, dtype=np.int64); pid = np.ascontiguousarray(point_id, dtype=np.int32)
        pts = np.ascontiguousarray(points, dtype=np.float64); pc = np.ascontiguousarray(p_c, dtype=np.float64)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        _check(self.L.vc_add_observation_tiles(self.h, len(tf), vp(tf), vp(tc), vp(off), vp(pts), len(pts), vp(pid), vp(pc)), "AddObservationTiles")

    def AddImuMeasurements(self, gyro, accel, time):
        time = np.ascontiguousarray(time, dtype=np.float64)
        _check(self.L.vc_add_imu(self.h, int(len(time)), _d(gyro), _d(accel), _d(time)), "AddImuMeasurements")

    def SetSigmas(self, g, a): _check(self.L.vc_set_sigmas(self.h, C.c_double(g), C.c_double(a)), "SetSigmas")
    def SetBiases(self, b): _check(self.L.vc_set_biases(self.h, _d(b)), "SetBiases")
    def SetGravity(self, g): _check(self.L.vc_set_gravity(self.h, _d(np.asarray(g, dtype=np.float64))), "SetGravity")   # engine-level (the reference has no setter)
    def SetScaleFactor(self, s): _check(self.L.vc_set_scale_factor(self.h, _d(s)), "SetScaleFactor")
    def SetTimeOffset(self, o): _check(self.L.vc_set_time_offset(self.h, C.c_double(o)), "SetTimeOffset")
    def SetFunctionTolerance(self, t): _check(self.L.vc_set_function_tolerance(self.h, C.c_double(t)), "SetFunctionTolerance")

    def SetOptimizationFlags(self, bias_active, inertial_active, rotation_only, optimize_time_offset):
        _check(self.L.vc_set_optimization_flags(self.h, int(bias_active), int(inertial_active), int(rotation_only), int(optimize_time_offset)), "SetOptimizationFlags")

    def SetTolerances(self, gradient_tolerance=1e-10, parameter_tolerance=1e-8):
        _check(self.L.vc_set_tolerances(self.h, C.c_double(gradient_tolerance), C.c_double(parameter_tolerance)), "SetTolerances")

    def SetMaxIters(self, m): _check(self.L.vc_set_max_iters(self.h, int(m)), "max_iters")
    def SetCalibrateImu(self, c): _check(self.L.vc_set_calibrate_imu(self.h, int(c)), "calibrate_imu")
    def SetRemoveOutliers(self, r, th=2.0): _check(self.L.vc_set_remove_outliers(self.h, int(r), C.c_double(th)), "remove_outliers")

    def Solve(self): return _check(self.L.vc_solve(self.h), "Solve")
    def Start(self): _check(self.L.vc_start(self.h), "Start")
    def SetStageLimit(self, n): _check(self.L.vc_set_stage_limit(self.h, int(n)), "SetStageLimit")
    def Resume(self): _check(self.L.vc_resume(self.h), "Resume")
    def IsRunning(self): return bool(self.L.vc_is_running(self.h))
    def Stop(self): _check(self.L.vc_stop(self.h), "Stop")
    def NumFrames(self): return self.L.vc_num_frames(self.h)
    def num_imu_blocks(self): return _check(self.L.vc_num_imu_blocks(self.h), "num_imu_blocks")
    def NumCameras(self): return self.L.vc_num_cameras(self.h)

    def GetCamera(self, c):
        K = np.zeros(10); n = C.c_int(0); T = np.zeros(7)
        _check(self.L.vc_get_camera(self.h, int(c), _d(K), C.byref(n), _d(T)), "GetCamera")
        return K[:n.value].copy(), T

    def GetFrame(self, f):
        T = np.zeros(7); v = np.zeros(3); t = C.c_double(0)
        _check(self.L.vc_get_frame(self.h, int(f), _d(T), _d(v), C.byref(t)), "GetFrame")
        return T, v, t.value

    def GetVelocities(self):
        n = self.NumFrames()
        v = np.zeros((n, 3))
        for f in range(n):
            v[f] = self.GetFrame(f)[1]
        return v

    def GetFrames(self):
        n = self.NumFrames()
        T = np.zeros((n, 7))
        for f in range(n):
            T[f] = self.GetFrame(f)[0]
        return T

    def GetBiases(self):
        b = np.zeros(6); _check(self.L.vc_get_biases(self.h, _d(b)), "GetBiases"); return b

    def GetScaleFactor(self):
        s = np.zeros(6); _check(self.L.vc_get_scale_factor(self.h, _d(s)), "GetScaleFactor"); return s

    def GetGravity(self):
        g = np.zeros(2); _check(self.L.vc_get_gravity(self.h, _d(g)), "GetGravity"); return g

    def time_offset(self): return self.L.vc_time_offset(self.h)
    def MeanSquaredError(self): return self.L.vc_mean_squared_error(self.h)

    def GetCameraProjRMSE(self):
        r = np.zeros(max(self.NumCameras(), 1)); _check(self.L.vc_get_camera_proj_rmse(self.h, _d(r)), "GetCameraProjRMSE")
        return r[:self.NumCameras()]

    def GetNumIterations(self): return self.L.vc_get_num_iterations(self.h)

    def imu_buffer(self):
        n = _check(self.L.vc_num_imu_measurements(self.h), "imu_buffer")
        g = np.zeros((n, 3)); a = np.zeros((n, 3)); t = np.zeros(n)
        _check(self.L.vc_get_imu_measurements(self.h, _d(g), _d(a), _d(t), n), "imu_buffer")
        return g, a, t

    def GetIntegrationPoses(self, frame_id):
        n = _check(self.L.vc_get_integration_poses(self.h, int(frame_id), None, 0), "GetIntegrationPoses")     # the count first
        out = np.zeros((max(n, 1), 11))
        if n > 0:
            _check(self.L.vc_get_integration_poses(self.h, int(frame_id), _d(out), n), "GetIntegrationPoses")
        return out[:n]

    def PrintResults(self):
        # the length first (any number of cameras); a worker started with Start() may change the values -- and with them the
        # length of the %.10g text -- between the two calls: some slack, and another round if that was not enough
        for _ in range(8):
            n = _check(self.L.vc_print_results(self.h, None, 0), "PrintResults")
            buf = C.create_string_buffer(n + 65)
            if self.L.vc_print_results(self.h, buf, n + 65) >= 0:
                return buf.value.decode()
        raise VicalibError("PrintResults: the text kept growing")
    def WriteCameraModels(self, path): _check(self.L.vc_write_camera_models(self.h, path.encode()), "WriteCameraModels")

    # ---- engine-level ------------------------------------------------------------------------
    def load_problem(self, prob, init=True):
        for c, m in enumerate(prob.cam_model):
            self.AddCamera(m, prob.cam_K_init[c] if init else prob.cam_K_gt[c], prob.cam_T_ck_init[c] if init else prob.cam_T_ck_gt[c],
                           prob.cfg.width, prob.cfg.height)
        T = prob.frame_T_wk_init if init else prob.frame_T_wk_gt
        for n in range(len(prob.frame_time)):
            self.AddFrame(T[n], prob.frame_time[n])
        if getattr(prob, "flat", None) is not None:
            tf, tc, off, ids, pix = prob.flat
            self.AddObservationTiles(tf, tc, off, prob.grid_points, ids, pix)
        else:
            for (f, c, ids, pix) in prob.tiles:
                self.AddObservations(f, c, prob.grid_points[ids], pix)
        if prob.imu_t is not None:
            self.AddImuMeasurements(prob.imu_gyro, prob.imu_accel, prob.imu_t)
        return self

    def trace(self):
        n = _check(self.L.vc_trace_len(self.h), "trace_len")
        out = np.zeros((max(n, 1), 10))
        _check(self.L.vc_get_trace(self.h, _d(out), n), "get_trace")
        return out[:n]

    def set_shard(self, rank, world, fn=None):
        self._cb = ALLREDUCE_FN(fn) if fn is not None else None
        _check(self.L.vc_set_shard(self.h, int(rank), int(world), self._cb, None), "set_shard")

    def set_shard_rccl(self, rank, world, group=None):
        """Frame sharding over the library's own RCCL communicator; the 128-byte id travels through torch.distributed."""
        import torch.distributed as dist
        buf = C.create_string_buffer(128)
        if rank == 0:
            _check(self.L.vc_rccl_unique_id(buf), "rccl_unique_id")
        box = [bytes(buf.raw)]
        if world > 1:
            dist.broadcast_object_list(box, src=0, group=group)
        rc = self.L.vc_set_shard_rccl(self.h, int(rank), int(world), C.create_string_buffer(box[0], 128))
        if rc != 0:          # say which RCCL call failed and why (vc_last_error) before the caller falls back to another transport
            raise VicalibError("set_shard_rccl: status %d: %s" % (rc, (self.L.vc_last_error() or b"").decode(errors="replace")))

    def set_shard_comm(self, comm):
        """Frame sharding over a communicator shared with the process's other calibrators (ShardComm); not owned by this calibrator."""
        rc = self.L.vc_set_shard_comm(self.h, comm.h)
        if rc != 0:
            raise VicalibError("set_shard_comm: status %d: %s" % (rc, (self.L.vc_last_error() or b"").decode(errors="replace")))

    def allreduce_calls(self): return int(self.L.vc_allreduce_calls(self.h))

    def pass_paths(self):
        """Which forms of the visual-inertial pass the uploaded problem runs (vc_pass_paths)."""
        out = (C.c_int * 6)()
        _check(self.L.vc_pass_paths(self.h, out), "pass_paths")
        return dict(fold_l0=out[0], back_path=out[1], early_gram=out[2], top_gram_launch=out[3], tail_deferred=out[4], shared_blocks_ahead=out[5])

    def chain_order(self):
        """Which levels of the chain elimination the uploaded problem eliminates odd-even inside a workgroup (vc_chain_order)."""
        n, top, oe = C.c_int(0), C.c_int(0), (C.c_int * 16)()
        _check(self.L.vc_chain_order(self.h, C.byref(n), oe, 16, C.byref(top)), "chain_order")
        return dict(n_levels=n.value, oe=[int(oe[l]) for l in range(n.value)], oe_top=top.value)

    def shard_info(self):
        """rank / world size the calibrator shards with and, for the library's own communicator, what RCCL reports (-1: none attached)."""
        v = [C.c_int(-1) for _ in range(4)]
        _check(self.L.vc_shard_info(self.h, *[C.byref(x) for x in v]), "shard_info")
        return dict(rank=v[0].value, world=v[1].value, rccl_ranks=v[2].value, rccl_rank=v[3].value)

    def stream(self): return self.L.vc_get_stream(self.h)
    def prepare(self): _check(self.L.vc_prepare(self.h), "prepare")
    def shared_dim(self): return _check(self.L.vc_shared_dim(self.h), "shared_dim")

    def linearize(self):
        self.prepare()
        n, D = self.NumFrames(), self.shared_dim()
        cost = C.c_double(0); H = np.zeros((n, 6, 6)); g = np.zeros((n, 6)); S = np.zeros((D, D)); gr = np.zeros(D); hd = np.zeros(D); gs = np.zeros(D)
        _check(self.L.vc_linearize(self.h, C.byref(cost), _d(H), _d(g), _d(S), _d(gr), _d(hd), _d(gs)), "linearize")
        return dict(cost=cost.value, Hpp=H, gp=g, S=S, g_red=gr, hss_diag=hd, g_s=gs)

    def step_hold(self, radius):
        """One LM pass at the current state with the decision withheld (vc_step_hold): the step it formed and the trial state, read out."""
        self.prepare()
        n, D, nc = self.NumFrames(), self.shared_dim(), self.NumCameras()
        cost = C.c_double(0); ds = np.zeros(max(D, 1)); sl = np.zeros(max(D, 1)); fl = np.zeros((n, 9))
        T = np.zeros((n, 7)); v = np.zeros((n, 3)); cams = np.zeros((max(nc, 1), 17)); imus = np.zeros(15)
        _check(self.L.vc_step_hold(self.h, C.c_double(radius), C.byref(cost), _d(ds), _d(sl), _d(fl), _d(T), _d(v), _d(cams), _d(imus)), "step_hold")
        return dict(cost=cost.value, delta_s=ds[:D], slam=sl[:D], frame_lam=fl, poses=T, vels=v, cams=cams[:nc], imus=imus)

    def evaluate(self):
        cost = C.c_double(0); sq = C.c_double(0)
        _check(self.L.vc_evaluate(self.h, C.byref(cost), C.byref(sq)), "evaluate")
        return cost.value, sq.value

    def run_iterations(self, iters):
        j = C.c_int(0); r = C.c_int(0)
        n = _check(self.L.vc_run_iterations(self.h, int(iters), C.byref(j), C.byref(r)), "run_iterations")
        return n, j.value, r.value

    def download_state(self):
        """The device's accepted state (where run_iterations left it) into what GetCamera / GetFrame / GetBiases / ... return."""
        _check(self.L.vc_download_state(self.h), "download_state")

    def time_kernels(self, reps=20):
        a = C.c_double(0); b = C.c_double(0)
        _check(self.L.vc_time_kernels(self.h, int(reps), C.byref(a), C.byref(b)), "time_kernels")
        return a.value, b.value

    def time_stages(self, reps=50):
        out = np.zeros(6)
        _check(self.L.vc_time_stages(self.h, int(reps), _d(out)), "time_stages")
        return dict(zip(["jac", "frame_schur", "-", "reduced", "trial", "final"], (out * 1e3).tolist()))

    def set_kernel_timing(self, on=True): _check(self.L.vc_set_kernel_timing(self.h, int(on)), "set_kernel_timing")

    def sync_timeouts(self):
        """Device-flag hand-overs that ran into their bound so far (each one reported on stderr, the solve resumed with events)."""
        return int(self.L.vc_sync_timeouts(self.h))

    def kernel_timing(self):
        """{launch group: (launches, average ms)} of the solves run since set_kernel_timing(True)."""
        names = C.create_string_buffer(2048); tot = np.zeros(64); cnt = np.zeros(64, dtype=np.int64)
        n = _check(self.L.vc_get_kernel_timing(self.h, names, len(names), _d(tot), cnt.ctypes.data_as(C.c_void_p), 64), "kernel_timing")
        keys = names.value.decode().split(";") if n else []
        return {k: (int(cnt[i]), float(tot[i] / cnt[i])) for i, k in enumerate(keys)}

    def imu_weights(self):
        ns = self.num_imu_blocks()
        W = np.zeros((ns, 9, 9))
        _check(self.L.vc_get_imu_weights(self.h, _d(W)), "imu_weights")
        return W

    def GetSolutionCovariance(self):
        """(covariance n x n, block names) of q_ck / p_ck / params of every camera at the current state
        (GetSolutionCovariance, vicalibrator.h:802-857; names as in :563, :569, :596)."""
        n = _check(self.L.vc_solution_covariance_dim(self.h), "solution_covariance_dim")
        cov = np.zeros((n, n)); m = C.c_int(0)
        _check(self.L.vc_get_solution_covariance(self.h, _d(cov), n, C.byref(m)), "solution_covariance")
        buf = C.create_string_buffer(64 * max(1, self.NumCameras()))
        _check(self.L.vc_get_solution_covariance_names(self.h, buf, len(buf)), "solution_covariance_names")
        return cov, buf.value.decode().split()

    def imu_blocks(self):
        ns = self.num_imu_blocks()
        H = np.zeros((ns, 33, 33)); g = np.zeros((ns, 33)); c = np.zeros(ns)
        _check(self.L.vc_get_imu_blocks(self.h, _d(H), _d(g), _d(c)), "imu_blocks")
        return H, g, c

    def report(self, bins=(16, 12), corners=True):
        """Residual report at the current state (vc_report_*): per corner (caller's order) r [n, 2], frame, camera, flags (bit 0 dropped by
        the outlier stage, bit 1 kept with one copy fewer); per view frame, camera, count, removed, sum_sq, max_err, worst_corner; per
        camera the error map [bins_y, bins_x, 4] = count, sum ru, sum rv, sum |r|^2; per IMU block whitened [9], unwhitened [9], flags."""
        bx, by = int(bins[0]), int(bins[1])
        _check(self.L.vc_report_compute(self.h, bx, by), "report_compute")
        vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        out = {"bins": (bx, by)}
        if corners:
            n = _check(self.L.vc_report_num_corners(self.h), "report_num_corners")
            r = np.zeros((n, 2)); fr = np.zeros(n, dtype=np.int32); cm = np.zeros(n, dtype=np.int32); fl = np.zeros(n, dtype=np.uint8)
            _check(self.L.vc_report_corners(self.h, C.c_longlong(0), C.c_longlong(n), _d(r), vp(fr), vp(cm), vp(fl)), "report_corners")
            out.update(r=r, frame=fr, camera=cm, flags=fl)
        nv = _check(self.L.vc_report_num_views(self.h), "report_num_views")
        v = dict(frame=np.zeros(nv, dtype=np.int32), camera=np.zeros(nv, dtype=np.int32), count=np.zeros(nv, dtype=np.int32), removed=np.zeros(nv, dtype=np.int32),
                 sum_sq=np.zeros(nv), max_err=np.zeros(nv), worst_corner=np.zeros(nv, dtype=np.int64))
        _check(self.L.vc_report_views(self.h, vp(v["frame"]), vp(v["camera"]), vp(v["count"]), vp(v["removed"]), vp(v["sum_sq"]), vp(v["max_err"]),
                                      vp(v["worst_corner"])), "report_views")
        out["views"] = v
        maps = np.zeros((self.NumCameras(), by, bx, 4))
        for c in range(self.NumCameras()):
            _check(self.L.vc_report_error_map(self.h, c, vp(maps[c])), "report_error_map")
        out["maps"] = maps
        nb = _check(self.L.vc_report_num_imu_blocks(self.h), "report_num_imu_blocks")
        w = np.zeros((nb, 9)); u = np.zeros((nb, 9)); f = np.zeros(nb, dtype=np.uint8)
        _check(self.L.vc_report_imu(self.h, vp(w), vp(u), vp(f)), "report_imu")
        out["imu"] = dict(whitened=w, unwhitened=u, flags=f)
        return out

    def time_report_sweeps(self, reps=20):
        """Average ms per launch of the sweeps of the last report(): vision, error map, IMU (vc_time_report_sweeps)."""
        out = np.zeros(3)
        _check(self.L.vc_time_report_sweeps(self.h, int(reps), _d(out)), "time_report_sweeps")
        return dict(vision=out[0], error_map=out[1], imu=out[2])

    HOLDOUT_STATUS = ("converged", "max_iters", "underdetermined", "no_seed", "failed")

    def HoldoutClear(self): _check(self.L.vc_holdout_clear(self.h), "HoldoutClear")

    def HoldoutAddTiles(self, tile_frame, tile_cam, tile_off, points, point_id, p_c):
        """Held-out views in the layout of AddObservationTiles; tile_frame numbers the held-out frames (vc_holdout_add_tiles)."""
        tf = np.ascontiguousarray(tile_frame, dtype=np.int32); tc = np.ascontiguousarray(tile_cam, dtype=np.int32)
        off = np.ascontiguousarray(tile_off, dtype=np.int64); pid = np.ascontiguousarray(point_id, dtype=np.int32)
        pts = np.ascontiguousarray(points, dtype=np.float64); pc = np.ascontiguousarray(p_c, dtype=np.float64)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        _check(self.L.vc_holdout_add_tiles(self.h, len(tf), vp(tf), vp(tc), vp(off), vp(pts), len(pts), vp(pid), vp(pc)), "HoldoutAddTiles")

    def HoldoutCompute(self, seeds=None, max_iters=0, corners=True):
        """Refit the held-out frames' poses with the cameras frozen and score them (vc_holdout_*).  seeds: [n_frames, 7] T_wk or None
        (PnP seeds).  Returns frames = T_wk [n, 7], status, iterations, cost0, cost, behind; views = frame, camera, count, sum_sq, max_err,
        worst_corner; per corner (caller's order) r [n, 2], frame, camera; per camera rmse and count over the fitted frames."""
        sp = None
        if seeds is not None:
            seeds = np.ascontiguousarray(seeds, dtype=np.float64).reshape(-1, 7)
            sp = seeds.ctypes.data_as(C.c_void_p)
        _check(self.L.vc_holdout_compute(self.h, sp, int(max_iters)), "HoldoutCompute")
        return self.HoldoutResults(corners)

    def HoldoutResults(self, corners=True):
        vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        nf = _check(self.L.vc_holdout_num_frames(self.h), "holdout_num_frames")
        f = dict(T_wk=np.zeros((nf, 7)), status=np.zeros(nf, dtype=np.int32), iterations=np.zeros(nf, dtype=np.int32), cost0=np.zeros(nf), cost=np.zeros(nf),
                 behind=np.zeros(nf, dtype=np.int32))
        _check(self.L.vc_holdout_frames(self.h, vp(f["T_wk"]), vp(f["status"]), vp(f["iterations"]), vp(f["cost0"]), vp(f["cost"]), vp(f["behind"])), "holdout_frames")
        nv = _check(self.L.vc_holdout_num_views(self.h), "holdout_num_views")
        v = dict(frame=np.zeros(nv, dtype=np.int32), camera=np.zeros(nv, dtype=np.int32), count=np.zeros(nv, dtype=np.int32), sum_sq=np.zeros(nv), max_err=np.zeros(nv),
                 worst_corner=np.zeros(nv, dtype=np.int64))
        _check(self.L.vc_holdout_views(self.h, vp(v["frame"]), vp(v["camera"]), vp(v["count"]), vp(v["sum_sq"]), vp(v["max_err"]), vp(v["worst_corner"])), "holdout_views")
        out = dict(frames=f, views=v)
        if corners:
            n = _check(self.L.vc_holdout_num_corners(self.h), "holdout_num_corners")
            r = np.zeros((n, 2)); fr = np.zeros(n, dtype=np.int32); cm = np.zeros(n, dtype=np.int32)
            _check(self.L.vc_holdout_corners(self.h, C.c_longlong(0), C.c_longlong(n), vp(r), vp(fr), vp(cm)), "holdout_corners")
            out.update(r=r, frame=fr, camera=cm)
        nc = self.NumCameras()
        rm = np.zeros(max(nc, 1)); cnt = np.zeros(max(nc, 1), dtype=np.int64)
        _check(self.L.vc_holdout_camera_rmse(self.h, vp(rm), vp(cnt)), "holdout_camera_rmse")
        out.update(rmse=rm[:nc], count=cnt[:nc])
        return out

    def time_holdout(self, reps=20):
        """Average ms per launch of the kernels of the last HoldoutCompute: pose refit, residual sweep (vc_time_holdout)."""
        out = np.zeros(2)
        _check(self.L.vc_time_holdout(self.h, int(reps), _d(out)), "time_holdout")
        return dict(pose=out[0], residuals=out[1])

    def debug_stamps(self):
        out = np.zeros(32, dtype=np.int64)
        _check(self.L.vc_get_debug_stamps(self.h, out.ctypes.data_as(C.c_void_p)), "debug_stamps")
        return out

    def num_observations(self): return int(self.L.vc_num_observations(self.h))
    def num_tiles(self): return int(self.L.vc_num_tiles(self.h))


class ConicDetector:
    """The image front-end's first slice (include/vicalib_amd.h: vc_detector_*): what VicalibTask's image_processing_[i] /
    conic_finder_[i] pair does per image (vicalib-task.cc:264-270) -- adaptive threshold, dot components, one conic per dot --
    on the GPU.  find(image) -> centres [n, 2] (x, y)."""

    def __init__(self, width, height, device=0):
        self.L = load()
        self.h = C.c_void_p()
        _check(self.L.vc_detector_create(int(device), int(width), int(height), C.byref(self.h)), "detector_create")
        self.w, self.hh = int(width), int(height)

    def close(self):
        if getattr(self, "h", None):
            self.L.vc_detector_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def set_params(self, black_on_white=True, at_threshold=0.9, at_window_ratio=30.0, conic_min_area=4.0, conic_min_density=0.6, conic_min_aspect=0.2):
        _check(self.L.vc_detector_set_params(self.h, int(black_on_white), C.c_double(at_threshold), C.c_double(at_window_ratio), C.c_double(conic_min_area),
                                             C.c_double(conic_min_density), C.c_double(conic_min_aspect)), "detector_set_params")

    def find(self, image, max_conics=4096):
        image = np.ascontiguousarray(image, dtype=np.uint8)
        assert image.shape == (self.hh, self.w)
        out = np.empty((max_conics, 2)); n = C.c_int(0)
        _check(self.L.vc_detector_find(self.h, image.ctypes.data_as(C.c_void_p), int(image.strides[0]), _d(out), int(max_conics), C.byref(n)), "detector_find")
        return out[:min(n.value, max_conics)]

    def find_conics(self, image, max_conics=4096):
        """-> (centres [n, 2], conics [n, 3, 3] (x^T C x = 0 on the edge, unit Frobenius norm), boxes [n, 4] (x0, y0, x1, y1 inclusive))"""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        assert image.shape == (self.hh, self.w)
        out = np.zeros((max_conics, 2)); con = np.zeros((max_conics, 9)); box = np.zeros((max_conics, 4), dtype=np.int32); n = C.c_int(0)
        _check(self.L.vc_detector_find_conics(self.h, image.ctypes.data_as(C.c_void_p), int(image.strides[0]), _d(out), _d(con),
                                              box.ctypes.data_as(C.c_void_p), int(max_conics), C.byref(n)), "detector_find_conics")
        k = min(n.value, max_conics)
        return out[:k], con[:k].reshape(-1, 3, 3), box[:k]


_hip = None


def hip_runtime():
    """The HIP runtime the library itself is linked against, for the few runtime calls tests and tools make beside the C ABI (device buffers,
    a reference copy): the very shared object that is mapped into this process, with argument types declared."""
    global _hip
    if _hip is None:
        load()
        with open("/proc/self/maps") as f:
            path = next((line.split()[-1] for line in f if "libamdhip64" in line), None)
        if path is None:
            raise VicalibError("the HIP runtime is not mapped into this process")
        H = C.CDLL(path)
        vp, sz = C.c_void_p, C.c_size_t
        H.hipMalloc.argtypes = [C.POINTER(vp), sz]
        H.hipFree.argtypes = [vp]
        H.hipMemcpy.argtypes = [vp, vp, sz, C.c_int]
        H.hipMemcpyAsync.argtypes = [vp, vp, sz, C.c_int, vp]
        H.hipMemset.argtypes = [vp, C.c_int, sz]
        H.hipDeviceSynchronize.argtypes = []
        H.hipEventCreate.argtypes = [C.POINTER(vp)]
        H.hipEventDestroy.argtypes = [vp]
        H.hipEventRecord.argtypes = [vp, vp]
        H.hipEventSynchronize.argtypes = [vp]
        H.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
        _hip = H
    return _hip


class DeviceBuffer:
    """A device allocation that holds a numpy array's bytes (hipMalloc + hipMemcpy): what a caller of the *_device entry points has."""

    def __init__(self, arr):
        arr = np.ascontiguousarray(arr)
        self.shape, self.dtype, self.nbytes, self.ptr = arr.shape, arr.dtype, arr.nbytes, C.c_void_p()
        H = hip_runtime()
        if H.hipMalloc(C.byref(self.ptr), arr.nbytes) != 0 or H.hipMemcpy(self.ptr, arr.ctypes.data, arr.nbytes, 1) != 0:      # 1 = hipMemcpyHostToDevice
            raise VicalibError("DeviceBuffer: hipMalloc / hipMemcpy failed")

    def numpy(self):
        """the buffer's content, after a device-wide synchronisation"""
        out = np.zeros(self.shape, dtype=self.dtype)
        H = hip_runtime()
        if H.hipDeviceSynchronize() != 0 or H.hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) != 0:      # 2 = hipMemcpyDeviceToHost
            raise VicalibError("DeviceBuffer: hipMemcpy failed")
        return out

    def free(self):
        if self.ptr:
            hip_runtime().hipFree(self.ptr)
            self.ptr = C.c_void_p()


def _model_id(model):
    from .synth import MODEL_IDS
    return MODEL_IDS[model] if isinstance(model, str) else int(model)


class Undistorter:
    """Using a calibration (include/vicalib_amd.h: vc_undistort*): images and pixels of a calibrated source camera mapped into an ideal
    pinhole destination camera dst_linear = [fu, fv, u0, v0] of dst_size = (w, h), rotated against the source by R_ds (3 x 3, source rays ->
    destination rays; None = identity).  The lookup table is built once, on the GPU.  map() -> (map [h, w, 2] float32, valid [h, w] bool);
    images(arr) -> undistorted uint8 images; points(px) -> (destination pixels [n, 2], valid [n] bool)."""

    def __init__(self, model, params, src_size, dst_linear, dst_size=None, R_ds=None, fill=0, device=0, _camera_of=None):
        self.L = load()
        self.h = C.c_void_p()
        dst_size = tuple(src_size if dst_size is None else dst_size)
        dl = np.ascontiguousarray(dst_linear, dtype=np.float64)
        assert dl.shape == (4,)
        R = None if R_ds is None else np.ascontiguousarray(R_ds, dtype=np.float64).reshape(3, 3)
        Rp = None if R is None else _d(R)
        if _camera_of is not None:
            cal, cam = _camera_of
            _check(self.L.vc_undistorter_create_for_camera(cal.h, int(cam), _d(dl), int(dst_size[0]), int(dst_size[1]), Rp, int(fill), C.byref(self.h)),
                   "undistorter_create_for_camera")
        else:
            params = np.ascontiguousarray(params, dtype=np.float64)
            _check(self.L.vc_undistorter_create(int(device), _model_id(model), _d(params), len(params), int(src_size[0]), int(src_size[1]), _d(dl),
                                                int(dst_size[0]), int(dst_size[1]), Rp, int(fill), C.byref(self.h)), "undistorter_create")
        self.src_size = (int(src_size[0]), int(src_size[1]))
        self.dst_size = (int(dst_size[0]), int(dst_size[1]))
        self._borrowed = False

    @classmethod
    def _borrow(cls, handle, src_size, dst_size):
        """A side of a Rectifier: the handle belongs to the rectifier and is never destroyed here."""
        u = cls.__new__(cls)
        u.L, u.h = load(), C.c_void_p(handle)
        u.src_size = (int(src_size[0]), int(src_size[1])); u.dst_size = (int(dst_size[0]), int(dst_size[1]))
        u._borrowed = True
        return u

    @classmethod
    def for_camera(cls, cal, camera, src_size, dst_linear, dst_size=None, R_ds=None, fill=0):
        """For camera `camera` of a ViCalibrator as GetCamera returns it (src_size: the size it was added with)."""
        return cls(None, None, src_size, dst_linear, dst_size, R_ds, fill, _camera_of=(cal, camera))

    @staticmethod
    def fit_linear(model, params, src_size, dst_size=None, alpha=0.0):
        """Destination intrinsics [fu, fv, u0, v0] for identity rotation (vc_undistort_fit_linear; host code, needs no GPU): alpha = 0 every
        destination pixel has a source pixel, alpha = 1 every source pixel is kept."""
        dst_size = src_size if dst_size is None else dst_size
        params = np.ascontiguousarray(params, dtype=np.float64)
        out = np.zeros(4)
        _check(load().vc_undistort_fit_linear(_model_id(model), _d(params), len(params), int(src_size[0]), int(src_size[1]), int(dst_size[0]), int(dst_size[1]),
                                              C.c_double(alpha), _d(out)), "undistort_fit_linear")
        return out

    def close(self):
        if getattr(self, "h", None):
            if not getattr(self, "_borrowed", False):
                self.L.vc_undistorter_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def linear(self):
        dl = np.zeros(4); sz = (C.c_int * 2)()
        _check(self.L.vc_undistort_get_linear(self.h, _d(dl), sz), "undistort_get_linear")
        return dl, (sz[0], sz[1])

    def map(self):
        w, h = self.dst_size
        m = np.zeros((h, w, 2), dtype=np.float32); v = np.zeros((h, w), dtype=np.uint8)
        _check(self.L.vc_undistort_get_map(self.h, m.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)), "undistort_get_map")
        return m, v.astype(bool)

    def images(self, arr, out=None):
        """arr: uint8 [h, w] or [n, h, w]; rows and images may be strided (pixels of a row contiguous).  out: likewise at the destination size;
        only its pixels are written."""
        arr = np.asarray(arr)
        single = arr.ndim == 2
        a = arr[None] if single else arr
        assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[1:] == (self.src_size[1], self.src_size[0]), a.shape
        if a.strides[2] != 1 or a.strides[1] < a.shape[2] or (len(a) > 1 and a.strides[0] < a.strides[1] * a.shape[1]):
            a = np.ascontiguousarray(a)
        n = len(a)
        if out is None:
            o = np.zeros((n, self.dst_size[1], self.dst_size[0]), dtype=np.uint8)
        else:
            o = out[None] if out.ndim == 2 else out
            assert o.dtype == np.uint8 and o.shape == (n, self.dst_size[1], self.dst_size[0]) and o.strides[2] == 1 and o.flags.writeable
        _check(self.L.vc_undistort_images(self.h, n, C.c_void_p(a.ctypes.data), int(a.strides[1]), C.c_longlong(a.strides[0]), C.c_void_p(o.ctypes.data),
                                          int(o.strides[1]), C.c_longlong(o.strides[0])), "undistort_images")
        return o[0] if single else o

    def images_device(self, n, d_src, src_pitch, src_stride, d_dst, dst_pitch, dst_stride):
        """Device pointers (integers), enqueued on stream() without synchronisation (vc_undistort_images_device)."""
        _check(self.L.vc_undistort_images_device(self.h, int(n), C.c_void_p(int(d_src)), int(src_pitch), C.c_longlong(src_stride), C.c_void_p(int(d_dst)),
                                                 int(dst_pitch), C.c_longlong(dst_stride)), "undistort_images_device")

    def stream(self): return self.L.vc_undistort_stream(self.h)

    def points(self, px):
        px = np.ascontiguousarray(px, dtype=np.float64).reshape(-1, 2)
        out = np.zeros_like(px); valid = np.zeros(len(px), dtype=np.uint8)
        _check(self.L.vc_undistort_points(self.h, len(px), _d(px), out.ctypes.data_as(C.c_void_p), valid.ctypes.data_as(C.c_void_p)), "undistort_points")
        return out, valid.astype(bool)

    def time(self, n_images=64, reps=20):
        """Average ms per launch: map build, remap of n_images device-resident images, 65536 points (vc_time_undistort)."""
        out = np.zeros(3)
        _check(self.L.vc_time_undistort(self.h, int(n_images), int(reps), _d(out)), "time_undistort")
        return dict(map=out[0], remap=out[1], points=out[2])


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


class Rectifier:
    """Using the calibration of a pair (include/vicalib_amd.h: vc_stereo_*, vc_rectif*): cameras a and b -- (model, params, (w, h), T_ck) each --
    rotated into a common frame with one pinhole camera dst_linear of dst_size for both (dst_linear None: fitted at alpha).  rotations,
    fit_linear and match_tiles are host code and need no GPU.  side(0 / 1) -> that side's Undistorter (borrowed); pairs(a, b) -> the two
    rectified image batches; check(...) -> the stereo consistency check; time(reps) -> ms per launch of the last check's sweep."""

    def __init__(self, cam_a, cam_b, dst_size=None, dst_linear=None, alpha=0.0, fill=0, device=0, _cameras_of=None):
        self.L = load()
        self.h = C.c_void_p()
        dl = None if dst_linear is None else _d(np.ascontiguousarray(dst_linear, dtype=np.float64).reshape(4))
        if _cameras_of is not None:
            cal, a, b, size_a, size_b = _cameras_of
            dst_size = size_a if dst_size is None else dst_size
            _check(self.L.vc_rectifier_create_for_cameras(cal.h, int(a), int(b), dl, int(dst_size[0]), int(dst_size[1]), C.c_double(alpha), int(fill),
                                                          C.byref(self.h)), "rectifier_create_for_cameras")
        else:
            (ma, Ka, size_a, Ta), (mb, Kb, size_b, Tb) = cam_a, cam_b
            Ka = np.ascontiguousarray(Ka, dtype=np.float64); Kb = np.ascontiguousarray(Kb, dtype=np.float64)
            dst_size = size_a if dst_size is None else dst_size
            _check(self.L.vc_rectifier_create(int(device), _model_id(ma), _d(Ka), len(Ka), int(size_a[0]), int(size_a[1]), _d(Ta), _model_id(mb), _d(Kb), len(Kb),
                                              int(size_b[0]), int(size_b[1]), _d(Tb), dl, int(dst_size[0]), int(dst_size[1]), C.c_double(alpha), int(fill),
                                              C.byref(self.h)), "rectifier_create")
        self.src_sizes = ((int(size_a[0]), int(size_a[1])), (int(size_b[0]), int(size_b[1])))
        self.dst_size = (int(dst_size[0]), int(dst_size[1]))
        self._sides = [None, None]

    @classmethod
    def for_cameras(cls, cal, cam_a, cam_b, size_a, size_b=None, dst_size=None, dst_linear=None, alpha=0.0, fill=0):
        """For two cameras of a ViCalibrator as GetCamera returns them (size_a / size_b: the sizes they were added with)."""
        return cls(None, None, dst_size, dst_linear, alpha, fill, _cameras_of=(cal, cam_a, cam_b, size_a, size_a if size_b is None else size_b))

    @staticmethod
    def rotations(T_ck_a, T_ck_b):
        """-> (R_ds_a, R_ds_b, signed baseline) (vc_stereo_rectify_rotations)"""
        Ra = np.zeros((3, 3)); Rb = np.zeros((3, 3)); b = C.c_double(0)
        _check(load().vc_stereo_rectify_rotations(_d(T_ck_a), _d(T_ck_b), _d(Ra), _d(Rb), C.byref(b)), "stereo_rectify_rotations")
        return Ra, Rb, b.value

    @staticmethod
    def fit_linear(cam_a, R_ds_a, cam_b, R_ds_b, dst_size=None, alpha=0.0):
        """cam = (model, params, (w, h)) -> [fu, fv, u0, v0] common to both sides (vc_stereo_fit_linear)"""
        (ma, Ka, size_a), (mb, Kb, size_b) = cam_a[:3], cam_b[:3]
        Ka = np.ascontiguousarray(Ka, dtype=np.float64); Kb = np.ascontiguousarray(Kb, dtype=np.float64)
        dst_size = size_a if dst_size is None else dst_size
        out = np.zeros(4)
        Ra = np.ascontiguousarray(R_ds_a, dtype=np.float64).reshape(3, 3); Rb = np.ascontiguousarray(R_ds_b, dtype=np.float64).reshape(3, 3)
        _check(load().vc_stereo_fit_linear(_model_id(ma), _d(Ka), len(Ka), int(size_a[0]), int(size_a[1]), _d(Ra), _model_id(mb), _d(Kb), len(Kb), int(size_b[0]),
                                           int(size_b[1]), _d(Rb), int(dst_size[0]), int(dst_size[1]), C.c_double(alpha), _d(out)), "stereo_fit_linear")
        return out

    @staticmethod
    def match_tiles(tile_frame, tile_cam, tile_off, point_id, cam_a=0, cam_b=1):
        """-> (frames [F], frame_off [F + 1], pos_a [n], pos_b [n]): per frame that has both cameras the positions of the corners with equal point
        id, ordered by frame, then point id (vc_match_tiles)"""
        L = load()
        tf = np.ascontiguousarray(tile_frame, dtype=np.int32); tc = np.ascontiguousarray(tile_cam, dtype=np.int32)
        off = _i64(tile_off); ids = np.ascontiguousarray(point_id, dtype=np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        nf = C.c_int(0); n = C.c_longlong(0)
        _check(L.vc_match_tiles(len(tf), p(tf), p(tc), p(off), p(ids), int(cam_a), int(cam_b), C.byref(nf), C.byref(n), None, None, None, None), "match_tiles")
        frames = np.zeros(nf.value, dtype=np.int32); foff = np.zeros(nf.value + 1, dtype=np.int64)
        pa = np.zeros(n.value, dtype=np.int64); pb = np.zeros(n.value, dtype=np.int64)
        _check(L.vc_match_tiles(len(tf), p(tf), p(tc), p(off), p(ids), int(cam_a), int(cam_b), C.byref(nf), C.byref(n), p(frames), p(foff), p(pa), p(pb)), "match_tiles")
        return frames, foff, pa, pb

    def close(self):
        if getattr(self, "h", None):
            for u in self._sides:
                if u is not None:
                    u.close()
            self.L.vc_rectifier_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def side(self, k):
        if self._sides[k] is None:
            self._sides[k] = Undistorter._borrow(self.L.vc_rectifier_side(self.h, int(k)), self.src_sizes[k], self.dst_size)
        return self._sides[k]

    def get(self):
        """-> dict(R_ds_a, R_ds_b, dst_linear, dst_size, baseline, T_ck_rect_a, T_ck_rect_b)"""
        Ra = np.zeros((3, 3)); Rb = np.zeros((3, 3)); dl = np.zeros(4); sz = (C.c_int * 2)(); b = C.c_double(0); Ta = np.zeros(7); Tb = np.zeros(7)
        _check(self.L.vc_rectifier_get(self.h, _d(Ra), _d(Rb), _d(dl), sz, C.byref(b), _d(Ta), _d(Tb)), "rectifier_get")
        return dict(R_ds_a=Ra, R_ds_b=Rb, dst_linear=dl, dst_size=(sz[0], sz[1]), baseline=b.value, T_ck_rect_a=Ta, T_ck_rect_b=Tb)

    def pairs(self, a, b):
        """a, b: uint8 [n, h, w] of the two sources (contiguous) -> the two rectified batches (vc_rectify_pairs)"""
        a = np.ascontiguousarray(a, dtype=np.uint8); b = np.ascontiguousarray(b, dtype=np.uint8)
        single = a.ndim == 2
        if single:
            a, b = a[None], b[None]
        n = len(a)
        assert len(b) == n and a.shape[1:] == self.src_sizes[0][::-1] and b.shape[1:] == self.src_sizes[1][::-1], (a.shape, b.shape)
        oa = np.zeros((n, self.dst_size[1], self.dst_size[0]), dtype=np.uint8); ob = np.zeros_like(oa)
        ll = C.c_longlong
        _check(self.L.vc_rectify_pairs(self.h, n, C.c_void_p(a.ctypes.data), int(a.strides[1]), ll(a.strides[0]), C.c_void_p(b.ctypes.data), int(b.strides[1]),
                                       ll(b.strides[0]), C.c_void_p(oa.ctypes.data), int(oa.strides[1]), ll(oa.strides[0]), C.c_void_p(ob.ctypes.data),
                                       int(ob.strides[1]), ll(ob.strides[0])), "rectify_pairs")
        return (oa[0], ob[0]) if single else (oa, ob)

    def check(self, frame_off, px_a, px_b, target=None):
        """The stereo consistency check (vc_rectify_check) -> dict: per pair `pairs` [n, 6] (dv, d, P, mean row) and `invalid` [n] bool; per frame
        count, n_invalid, sum_dv, sum_dv2, max_abs_dv, worst, mean_z, rigid_rms."""
        foff = _i64(frame_off); nf = len(foff) - 1
        n = int(foff[-1]) if nf >= 0 and len(foff) else 0
        pa = np.ascontiguousarray(px_a, dtype=np.float64).reshape(-1, 2); pb = np.ascontiguousarray(px_b, dtype=np.float64).reshape(-1, 2)
        assert len(pa) == n and len(pb) == n, (len(pa), len(pb), n)
        tg = None
        if target is not None:
            tg = np.ascontiguousarray(target, dtype=np.float64).reshape(-1, 3)
            assert len(tg) == n
        out = dict(pairs=np.zeros((n, 6)), invalid=np.zeros(n, dtype=np.uint8), count=np.zeros(nf, dtype=np.int32), n_invalid=np.zeros(nf, dtype=np.int32),
                   sum_dv=np.zeros(nf), sum_dv2=np.zeros(nf), max_abs_dv=np.zeros(nf), worst=np.zeros(nf, dtype=np.int64), mean_z=np.zeros(nf),
                   rigid_rms=np.zeros(nf))
        p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        _check(self.L.vc_rectify_check(self.h, nf, p(foff), p(pa), p(pb), None if tg is None else p(tg), p(out["pairs"]), p(out["invalid"]), p(out["count"]),
                                       p(out["n_invalid"]), p(out["sum_dv"]), p(out["sum_dv2"]), p(out["max_abs_dv"]), p(out["worst"]), p(out["mean_z"]),
                                       p(out["rigid_rms"])), "rectify_check")
        out["invalid"] = out["invalid"].astype(bool)
        return out

    def time(self, reps=20):
        ms = C.c_double(0)
        _check(self.L.vc_time_rectify_check(self.h, int(reps), C.byref(ms)), "time_rectify_check")
        return ms.value


class Comparer:
    """Two calibrations of one camera compared in pixel space (include/vicalib_amd.h: vc_compar*): cameras a and b -- (model, params) each -- of
    the same image `size` = (w, h), sampled on a lattice `grid` = (gx, gy).  run(fit_radius) fits the implied rotation over the samples within
    that normalised radius (fit_radius <= 0: none, the difference is taken at R_ba) and sweeps the difference d = project(b, R unproject(a, q)) - q;
    fit(), map(), summary() and rings(n) read the last run; time(reps) -> ms per launch of the rays, one fit sweep and the difference sweep."""

    def __init__(self, cam_a, cam_b, size, grid=(64, 48), device=0, _camera_of=None):
        self.L = load()
        self.h = C.c_void_p()
        mb, Kb = cam_b
        Kb = np.ascontiguousarray(Kb, dtype=np.float64)
        if _camera_of is not None:
            cal, cam = _camera_of
            _check(self.L.vc_comparer_create_for_camera(cal.h, int(cam), _model_id(mb), _d(Kb), len(Kb), int(grid[0]), int(grid[1]), C.byref(self.h)),
                   "comparer_create_for_camera")
        else:
            ma, Ka = cam_a
            Ka = np.ascontiguousarray(Ka, dtype=np.float64)
            _check(self.L.vc_comparer_create(int(device), _model_id(ma), _d(Ka), len(Ka), _model_id(mb), _d(Kb), len(Kb), int(size[0]), int(size[1]),
                                             int(grid[0]), int(grid[1]), C.byref(self.h)), "comparer_create")
        self.grid = (int(grid[0]), int(grid[1]))

    @classmethod
    def for_camera(cls, cal, camera, cam_b, grid=(64, 48)):
        """Camera a is camera `camera` of a ViCalibrator as GetCamera returns it, with the size it was added with."""
        return cls(None, cam_b, None, grid, _camera_of=(cal, camera))

    def close(self):
        if getattr(self, "h", None):
            self.L.vc_comparer_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def run(self, fit_radius=0.5, max_iters=0, R_ba=None):
        Rp = None if R_ba is None else _d(np.ascontiguousarray(R_ba, dtype=np.float64).reshape(3, 3))
        _check(self.L.vc_compare_run(self.h, C.c_double(fit_radius), int(max_iters), Rp), "compare_run")
        return self.fit()

    def fit(self):
        R = np.zeros((3, 3)); st, it, nf, nl = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0); c0, c1 = C.c_double(0), C.c_double(0)
        _check(self.L.vc_compare_get_fit(self.h, _d(R), C.byref(st), C.byref(it), C.byref(nf), C.byref(nl), C.byref(c0), C.byref(c1)), "compare_get_fit")
        return dict(R=R, status=st.value, iterations=it.value, n_fit=nf.value, n_left_out=nl.value, cost0=c0.value, cost=c1.value)

    def map(self):
        """-> (d [gy, gx, 2], a NaN pair at an invalid sample; flags [gy, gx] uint8)"""
        gx, gy = self.grid
        d = np.zeros((gy, gx, 2)); f = np.zeros((gy, gx), dtype=np.uint8)
        _check(self.L.vc_compare_get_map(self.h, d.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p)), "compare_get_map")
        return d, f

    def summary(self):
        n, bad, w = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        su, sv, sq, mx = C.c_double(0), C.c_double(0), C.c_double(0), C.c_double(0)
        _check(self.L.vc_compare_summary(self.h, C.byref(n), C.byref(bad), C.byref(su), C.byref(sv), C.byref(sq), C.byref(mx), C.byref(w)), "compare_summary")
        return dict(count=n.value, invalid=bad.value, sum_du=su.value, sum_dv=sv.value, sum_sq=sq.value, max_err=mx.value, worst=w.value)

    def rings(self, n_rings=8):
        n, bad = np.zeros(n_rings, dtype=np.int64), np.zeros(n_rings, dtype=np.int64)
        sq, mx = np.zeros(n_rings), np.zeros(n_rings)
        p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        _check(self.L.vc_compare_rings(self.h, int(n_rings), p(n), p(bad), p(sq), p(mx)), "compare_rings")
        return dict(count=n, invalid=bad, sum_sq=sq, max_err=mx)

    @staticmethod
    def extrinsics(T_ck_a0, T_ck_ac, T_ck_b0, T_ck_bc, R_0=None, R_c=None):
        """Camera c against camera 0 of rigs a and b (vc_compare_extrinsics; host code, needs no GPU) -> [angle, distance] compensated by the two
        implied rotations, then [angle, distance] plain."""
        out = np.zeros(4)
        Rp = [None if R is None else _d(np.ascontiguousarray(R, dtype=np.float64).reshape(3, 3)) for R in (R_0, R_c)]
        _check(load().vc_compare_extrinsics(_d(T_ck_a0), _d(T_ck_ac), _d(T_ck_b0), _d(T_ck_bc), Rp[0], Rp[1], _d(out)), "compare_extrinsics")
        return out

    def time(self, reps=20):
        out = np.zeros(3)
        _check(self.L.vc_time_compare(self.h, int(reps), _d(out)), "time_compare")
        return out


class Converter:
    """A calibrated camera converted to another camera model (include/vicalib_amd.h: vc_convert*): source camera a = (model, params) of image
    `size` = (w, h), the target `model_b`, sampled on a lattice `grid` = (gx, gy).  run(fit_radius) fits the target's intrinsics to a's rays over
    the samples within that normalised radius (>= 1: the whole image) and returns what get() reads; comparer() is a Comparer of a against the
    result (run it with fit_radius = 0 for the residual per sample); time(reps) -> ms per launch of the rays, one linearisation and one cost sweep."""

    def __init__(self, cam_a, model_b, size, grid=(64, 48), device=0, _camera_of=None):
        self.L = load()
        self.h = C.c_void_p()
        if _camera_of is not None:
            cal, cam = _camera_of
            _check(self.L.vc_converter_create_for_camera(cal.h, int(cam), _model_id(model_b), int(grid[0]), int(grid[1]), C.byref(self.h)), "converter_create_for_camera")
        else:
            ma, Ka = cam_a
            Ka = np.ascontiguousarray(Ka, dtype=np.float64)
            _check(self.L.vc_converter_create(int(device), _model_id(ma), _d(Ka), len(Ka), int(size[0]), int(size[1]), _model_id(model_b), int(grid[0]), int(grid[1]),
                                              C.byref(self.h)), "converter_create")
        self.grid = (int(grid[0]), int(grid[1]))

    @classmethod
    def for_camera(cls, cal, camera, model_b, grid=(64, 48)):
        """The source is camera `camera` of a ViCalibrator as GetCamera returns it, with the size it was added with."""
        return cls(None, model_b, None, grid, _camera_of=(cal, camera))

    def close(self):
        if getattr(self, "h", None):
            self.L.vc_converter_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def run(self, fit_radius=1.0, max_iters=0, start=None, free_mask=0):
        sp = None if start is None else _d(np.ascontiguousarray(start, dtype=np.float64))
        _check(self.L.vc_convert_run(self.h, C.c_double(fit_radius), int(max_iters), sp, C.c_uint(int(free_mask))), "convert_run")
        return self.get()

    def get(self):
        K = np.zeros(10); nk, st, it, nf, nl = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        c0, c1, mx, w = C.c_double(0), C.c_double(0), C.c_double(0), C.c_longlong(0)
        _check(self.L.vc_convert_get(self.h, _d(K), C.byref(nk), C.byref(st), C.byref(it), C.byref(nf), C.byref(nl), C.byref(c0), C.byref(c1), C.byref(mx), C.byref(w)),
               "convert_get")
        return dict(K=K[:nk.value].copy(), status=st.value, iterations=it.value, n_fit=nf.value, n_left_out=nl.value, cost0=c0.value, cost=c1.value,
                    max_err=mx.value, worst=w.value)

    def comparer(self):
        cmp = Comparer.__new__(Comparer)
        cmp.L, cmp.h, cmp.grid = self.L, C.c_void_p(), self.grid
        _check(self.L.vc_convert_comparer(self.h, C.byref(cmp.h)), "convert_comparer")
        return cmp

    def time(self, reps=20):
        out = np.zeros(3)
        _check(self.L.vc_time_convert(self.h, int(reps), _d(out)), "time_convert")
        return out


class Uncertainty:
    """The projection uncertainty of one calibrated camera mapped over its image (include/vicalib_amd.h: vc_uncertainty*): camera = (model,
    params) of image `size` = (w, h), sampled on a lattice `grid` = (gx, gy).  run(cov, sigma_px, fit_radius) takes a covariance of the
    intrinsics (None: the calibrator's, on a handle made by for_camera), removes the rotation the extrinsics would absorb -- fitted over the
    samples within fit_radius; <= 0: none -- and maps Sigma = sigma_px^2 J cov J^T per sample; fit(), map(), summary() and rings(n) read the
    last run; time(reps) -> ms per launch of the rays, the sweep of G and C and the map sweep."""

    def __init__(self, camera, size, grid=(64, 48), device=0, _camera_of=None):
        self.L = load()
        self.h = C.c_void_p()
        if _camera_of is not None:
            cal, cam = _camera_of
            _check(self.L.vc_uncertainty_create_for_camera(cal.h, int(cam), int(grid[0]), int(grid[1]), C.byref(self.h)), "uncertainty_create_for_camera")
            self.nk = len(cal.GetCamera(cam)[0])
        else:
            m, K = camera
            K = np.ascontiguousarray(K, dtype=np.float64)
            _check(self.L.vc_uncertainty_create(int(device), _model_id(m), _d(K), len(K), int(size[0]), int(size[1]), int(grid[0]), int(grid[1]), C.byref(self.h)),
                   "uncertainty_create")
            self.nk = len(K)
        self.grid = (int(grid[0]), int(grid[1]))

    @classmethod
    def for_camera(cls, cal, camera, grid=(64, 48)):
        """Camera `camera` of a ViCalibrator as GetCamera returns it, with the size it was added with and its params block of
        GetSolutionCovariance() at the current state as the handle's covariance."""
        return cls(None, None, grid, _camera_of=(cal, camera))

    def close(self):
        if getattr(self, "h", None):
            self.L.vc_uncertainty_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def run(self, cov=None, sigma_px=1.0, fit_radius=0.5):
        cp = None
        if cov is not None:
            cov = np.ascontiguousarray(cov, dtype=np.float64)
            if cov.shape != (self.nk, self.nk):
                raise VicalibError("uncertainty_run failed: VC_ERR_BAD_ARG (cov is not nk x nk)")
            cp = _d(cov)
        _check(self.L.vc_uncertainty_run(self.h, cp, C.c_double(sigma_px), C.c_double(fit_radius)), "uncertainty_run")
        return self.fit()

    def fit(self):
        M = np.zeros((3, self.nk)); G = np.zeros((3, 3)); nf = C.c_int(0)
        _check(self.L.vc_uncertainty_get_fit(self.h, _d(M), _d(G), C.byref(nf)), "uncertainty_get_fit")
        return dict(M=M, G=G, n_fit=nf.value)

    def map(self):
        """-> (sigma [gy, gx, 3] = (s_uu, s_uv, s_vv), a NaN triple at an invalid sample; flags [gy, gx] uint8)"""
        gx, gy = self.grid
        s = np.zeros((gy, gx, 3)); f = np.zeros((gy, gx), dtype=np.uint8)
        _check(self.L.vc_uncertainty_get_map(self.h, s.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p)), "uncertainty_get_map")
        return s, f

    def summary(self):
        n, bad, w = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        sv, mx = C.c_double(0), C.c_double(0)
        _check(self.L.vc_uncertainty_summary(self.h, C.byref(n), C.byref(bad), C.byref(sv), C.byref(mx), C.byref(w)), "uncertainty_summary")
        return dict(count=n.value, invalid=bad.value, sum_var=sv.value, max_lam=mx.value, worst=w.value)

    def rings(self, n_rings=8):
        n, bad = np.zeros(n_rings, dtype=np.int64), np.zeros(n_rings, dtype=np.int64)
        sv, mx = np.zeros(n_rings), np.zeros(n_rings)
        p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        _check(self.L.vc_uncertainty_rings(self.h, int(n_rings), p(n), p(bad), p(sv), p(mx)), "uncertainty_rings")
        return dict(count=n, invalid=bad, sum_var=sv, max_lam=mx)

    def time(self, reps=20):
        out = np.zeros(3)
        _check(self.L.vc_time_uncertainty(self.h, int(reps), _d(out)), "time_uncertainty")
        return out


class StereoUncertainty:
    """The row and depth uncertainty of a calibrated stereo pair mapped over its rectified image (include/vicalib_amd.h:
    vc_stereo_uncertainty*): cameras a and b -- (model, params) of image size_a / size_b at T_ck_a / T_ck_b --, a destination pinhole
    dst_linear of dst_size held fixed (None: fitted at alpha) and a lattice `grid` = (gx, gy) over the rectified image of a.
    run(cov, sigma_px, depths) takes the joint covariance of the pair in the layout of a two-camera rig's GetSolutionCovariance() (None: the
    calibrator's, on a handle made by for_cameras) and maps (var_dv, var_d, var_Z) per sample and depth; map(), summary(), pose_sigma() and
    geometry() read the handle; time(reps) -> ms per launch of the two side sweeps and of the map sweep.  pose_jacobian is host code."""

    def __init__(self, cam_a, cam_b, size_a, size_b, T_ck_a, T_ck_b, dst_size=None, dst_linear=None, alpha=0.0, grid=(64, 48), device=0, _cameras_of=None):
        self.L = load()
        self.h = C.c_void_p()
        dl = None if dst_linear is None else _d(np.ascontiguousarray(dst_linear, dtype=np.float64).reshape(4))
        dst_size = size_a if dst_size is None else dst_size
        if _cameras_of is not None:
            cal, a, b = _cameras_of
            _check(self.L.vc_stereo_uncertainty_create_for_cameras(cal.h, int(a), int(b), dl, int(dst_size[0]), int(dst_size[1]), C.c_double(alpha), int(grid[0]),
                                                                   int(grid[1]), C.byref(self.h)), "stereo_uncertainty_create_for_cameras")
            self.n_cov = 14 + len(cal.GetCamera(a)[0]) + len(cal.GetCamera(b)[0])
        else:
            (ma, Ka), (mb, Kb) = cam_a, cam_b
            Ka = np.ascontiguousarray(Ka, dtype=np.float64); Kb = np.ascontiguousarray(Kb, dtype=np.float64)
            _check(self.L.vc_stereo_uncertainty_create(int(device), _model_id(ma), _d(Ka), len(Ka), int(size_a[0]), int(size_a[1]), _d(T_ck_a), _model_id(mb), _d(Kb),
                                                       len(Kb), int(size_b[0]), int(size_b[1]), _d(T_ck_b), dl, int(dst_size[0]), int(dst_size[1]), C.c_double(alpha),
                                                       int(grid[0]), int(grid[1]), C.byref(self.h)), "stereo_uncertainty_create")
            self.n_cov = 14 + len(Ka) + len(Kb)
        self.grid = (int(grid[0]), int(grid[1]))
        self.n_depths = 0

    @classmethod
    def for_cameras(cls, cal, cam_a, cam_b, size_a, dst_size=None, dst_linear=None, alpha=0.0, grid=(64, 48)):
        """For two cameras of a ViCalibrator as GetCamera returns them (size_a: the size camera a was added with), with the pair's rows and
        columns of GetSolutionCovariance() at the current state as the handle's covariance."""
        return cls(None, None, size_a, None, None, None, dst_size, dst_linear, alpha, grid, _cameras_of=(cal, cam_a, cam_b))

    @staticmethod
    def pose_jacobian(T_ck_a, T_ck_b):
        """-> W [7, 12] = d(w_a, w_b, baseline) / d(w_ck_a, dp_a, w_ck_b, dp_b) (vc_stereo_pose_jacobian)"""
        W = np.zeros((7, 12))
        _check(load().vc_stereo_pose_jacobian(_d(T_ck_a), _d(T_ck_b), W.ctypes.data_as(C.c_void_p)), "stereo_pose_jacobian")
        return W

    def close(self):
        if getattr(self, "h", None):
            self.L.vc_stereo_uncertainty_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def geometry(self):
        Ra, Rb, dl, W, b = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros(4), np.zeros((7, 12)), C.c_double(0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        _check(self.L.vc_stereo_uncertainty_get(self.h, p(Ra), p(Rb), p(dl), C.byref(b), p(W)), "stereo_uncertainty_get")
        return dict(R_ds_a=Ra, R_ds_b=Rb, dst_linear=dl, baseline=b.value, W=W)

    def run(self, cov=None, sigma_px=1.0, depths=(1.0,)):
        cp = None
        if cov is not None:
            cov = np.ascontiguousarray(cov, dtype=np.float64)
            if cov.shape != (self.n_cov, self.n_cov):
                raise VicalibError("stereo_uncertainty_run failed: VC_ERR_BAD_ARG (cov is not n x n, n = 14 + nk_a + nk_b)")
            cp = _d(cov)
        depths = np.ascontiguousarray(depths, dtype=np.float64).reshape(-1)
        self.n_depths = 0
        _check(self.L.vc_stereo_uncertainty_run(self.h, cp, C.c_double(sigma_px), _d(depths) if len(depths) else None, len(depths)), "stereo_uncertainty_run")
        self.n_depths = len(depths)
        return self

    def map(self):
        """-> (var [n_depths, gy, gx, 3] = (var_dv, var_d, var_Z), a NaN triple at an invalid sample; flags [n_depths, gy, gx] uint8)"""
        gx, gy = self.grid
        nd = max(self.n_depths, 1)
        v = np.zeros((nd, gy, gx, 3)); f = np.zeros((nd, gy, gx), dtype=np.uint8)
        _check(self.L.vc_stereo_uncertainty_get_map(self.h, v.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p)), "stereo_uncertainty_get_map")
        return v, f

    def summary(self, plane=None):
        """one depth plane's summary, or the list of all of them"""
        if plane is None:
            _check(self.L.vc_stereo_uncertainty_summary(self.h, 0, None, None, None, None, None, None, None), "stereo_uncertainty_summary")
            return [self.summary(k) for k in range(self.n_depths)]
        n, bad, w = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        s0, s1, s2, mx = C.c_double(0), C.c_double(0), C.c_double(0), C.c_double(0)
        _check(self.L.vc_stereo_uncertainty_summary(self.h, int(plane), C.byref(n), C.byref(bad), C.byref(s0), C.byref(s1), C.byref(s2), C.byref(mx), C.byref(w)),
               "stereo_uncertainty_summary")
        return dict(count=n.value, invalid=bad.value, sum_var_dv=s0.value, sum_var_d=s1.value, sum_var_z=s2.value, max_var_dv=mx.value, worst=w.value)

    def pose_sigma(self):
        """-> [7]: the variances of w_a (3), w_b (3) and of the baseline at the last run's covariance and sigma_px"""
        out = np.zeros(7)
        _check(self.L.vc_stereo_uncertainty_get_pose_sigma(self.h, out.ctypes.data_as(C.c_void_p)), "stereo_uncertainty_get_pose_sigma")
        return out

    def time(self, reps=20):
        out = np.zeros(2)
        _check(self.L.vc_time_stereo_uncertainty(self.h, int(reps), out.ctypes.data_as(C.c_void_p)), "time_stereo_uncertainty")
        return out


CAM_ROT_FREE, CAM_TRANS_FREE, CAM_K_FREE = 1, 2, 4


class Selector:
    """Greedy D-optimal selection of the most informative views (include/vicalib_amd.h: vc_selector*): cameras = [(model, params, T_ck, flags)]
    with the solver's flags (CAM_ROT_FREE | CAM_TRANS_FREE | CAM_K_FREE); add_tiles() and set_poses() give the candidate frames; run(k, start,
    prior) selects; result(), frames(), frame_information(f) and last_gains() read the last run; time(reps) -> ms per launch of the information
    sweep, one gain round and one pick."""

    def __init__(self, cameras, device=0, _calibrator=None):
        self.L = load()
        self.h = C.c_void_p()
        if _calibrator is not None:
            _check(self.L.vc_selector_create_for_calibrator(_calibrator.h, C.byref(self.h)), "selector_create_for_calibrator")
        else:
            n = len(cameras)
            model = np.array([_model_id(c[0]) for c in cameras], dtype=np.int32)
            nparams = np.array([len(c[1]) for c in cameras], dtype=np.int32)
            params = np.zeros((n, 10))
            for i, c in enumerate(cameras):
                params[i, :min(len(c[1]), 10)] = np.asarray(c[1], dtype=np.float64)[:10]
            T_ck = np.ascontiguousarray([c[2] for c in cameras], dtype=np.float64).reshape(n, 7)
            flags = np.array([int(c[3]) for c in cameras], dtype=np.int32)
            vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
            _check(self.L.vc_selector_create(int(device), n, vp(model), _d(params), vp(nparams), _d(T_ck), vp(flags), C.byref(self.h)), "selector_create")
        self.D = _check(self.L.vc_select_dim(self.h), "select_dim")
        self.n_frames = 0

    @classmethod
    def for_calibrator(cls, cal):
        """The cameras, flags, frame poses and observation tiles of a ViCalibrator at its host state."""
        s = cls(None, _calibrator=cal)
        s.n_frames = cal.NumFrames()
        return s

    def close(self):
        if getattr(self, "h", None):
            self.L.vc_selector_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def add_tiles(self, tile_frame, tile_cam, tile_off, points, point_id):
        tf = np.ascontiguousarray(tile_frame, dtype=np.int32); tc = np.ascontiguousarray(tile_cam, dtype=np.int32)
        off = np.ascontiguousarray(tile_off, dtype=np.int64); pid = np.ascontiguousarray(point_id, dtype=np.int32)
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        _check(self.L.vc_select_add_tiles(self.h, len(tf), vp(tf), vp(tc), vp(off), vp(pts), len(pts), vp(pid)), "select_add_tiles")

    def set_poses(self, T_wk):
        T = np.ascontiguousarray(T_wk, dtype=np.float64).reshape(-1, 7)
        _check(self.L.vc_select_set_poses(self.h, _d(T), len(T)), "select_set_poses")
        self.n_frames = len(T)

    def run(self, k, start=(), prior=1e-6):
        st = np.ascontiguousarray(start, dtype=np.int32)
        _check(self.L.vc_select_run(self.h, int(k), st.ctypes.data_as(C.c_void_p) if len(st) else None, len(st), C.c_double(prior)), "select_run")
        return self.result()

    def result(self):
        n = C.c_int(0); total = C.c_double(0)
        order = np.zeros(max(self.n_frames, 1), dtype=np.int32); gain = np.zeros(max(self.n_frames, 1)); cum = np.zeros(max(self.n_frames, 1))
        _check(self.L.vc_select_get(self.h, C.byref(n), order.ctypes.data_as(C.c_void_p), _d(gain), _d(cum), C.byref(total)), "select_get")
        return dict(order=order[:n.value].copy(), gain=gain[:n.value].copy(), cum=cum[:n.value].copy(), total=total.value)

    def frames(self):
        a = [np.zeros(max(self.n_frames, 1), dtype=np.int32) for _ in range(3)]
        _check(self.L.vc_select_frames(self.h, *[x.ctypes.data_as(C.c_void_p) for x in a]), "select_frames")
        return dict(status=a[0][:self.n_frames], corners=a[1][:self.n_frames], behind=a[2][:self.n_frames])

    def frame_information(self, frame):
        """-> (I_f [D, D] unscaled, scale [D])"""
        I = np.zeros((self.D, self.D)); s = np.zeros(self.D)
        _check(self.L.vc_select_frame_information(self.h, int(frame), _d(I), _d(s)), "select_frame_information")
        return I, s

    def last_gains(self):
        g = np.zeros(max(self.n_frames, 1))
        _check(self.L.vc_select_last_gains(self.h, _d(g)), "select_last_gains")
        return g[:self.n_frames]

    def time(self, reps=20):
        out = np.zeros(3)
        _check(self.L.vc_time_select(self.h, int(reps), _d(out)), "time_select")
        return out


class Registrar:
    """A depth image of one camera of the rig taken into another camera, and that camera's image taken into the depth camera's pixels
    (include/vicalib_amd.h: vc_regist*).  cam_s (the depth camera) and cam_d are (model, params, (w, h), T_ck) each; unit_src / unit_dst
    metres per count; kind "z" or "range"; splat "nearest" or "footprint".  depth(arr) -> (depth in D's pixels, index map, counters);
    color(depth, images) -> (images in S's pixels, visibility mask); points(rows) -> ((q_x, q_y, m_d / unit_dst) rows, valid)."""
    KINDS = {"z": 0, "range": 1}
    SPLATS = {"nearest": 0, "footprint": 1}

    def __init__(self, cam_s, cam_d, unit_src=0.001, unit_dst=0.001, kind="z", splat="nearest", device=0, _cameras_of=None):
        self.L = load()
        self.h = C.c_void_p()
        kind = self.KINDS.get(kind, kind); splat = self.SPLATS.get(splat, splat)
        if _cameras_of is not None:
            cal, s, d = _cameras_of
            _check(self.L.vc_registrar_create_for_cameras(cal.h, int(s), int(d), C.c_double(unit_src), C.c_double(unit_dst), int(kind), int(splat), C.byref(self.h)),
                   "registrar_create_for_cameras")
        else:
            (ms, Ks, size_s, Ts), (md, Kd, size_d, Td) = cam_s, cam_d
            Ks = np.ascontiguousarray(Ks, dtype=np.float64); Kd = np.ascontiguousarray(Kd, dtype=np.float64)
            _check(self.L.vc_registrar_create(int(device), _model_id(ms), _d(Ks), len(Ks), int(size_s[0]), int(size_s[1]), _d(Ts), _model_id(md), _d(Kd), len(Kd),
                                              int(size_d[0]), int(size_d[1]), _d(Td), C.c_double(unit_src), C.c_double(unit_dst), int(kind), int(splat),
                                              C.byref(self.h)), "registrar_create")
        g = self.get()                                       # the sizes are the handle's, whichever way it was made
        self.src_size, self.dst_size = g["src_size"], g["dst_size"]

    @classmethod
    def for_cameras(cls, cal, cam_s, cam_d, unit_src=0.001, unit_dst=0.001, kind="z", splat="nearest"):
        """For two cameras of a ViCalibrator, with the models, parameters, sizes and poses it holds for them."""
        return cls(None, None, unit_src, unit_dst, kind, splat, _cameras_of=(cal, cam_s, cam_d))

    def close(self):
        if getattr(self, "h", None):
            self.L.vc_registrar_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def get(self):
        """-> dict(R, t, src_size, dst_size, unit_src, unit_dst, kind, splat)"""
        R = np.zeros((3, 3)); t = np.zeros(3); ss = (C.c_int * 2)(); sd = (C.c_int * 2)(); units = np.zeros(2); kind = C.c_int(0); splat = C.c_int(0)
        _check(self.L.vc_register_get(self.h, _d(R), _d(t), ss, sd, _d(units), C.byref(kind), C.byref(splat)), "register_get")
        return dict(R=R, t=t, src_size=(ss[0], ss[1]), dst_size=(sd[0], sd[1]), unit_src=units[0], unit_dst=units[1], kind=kind.value, splat=splat.value)

    @staticmethod
    def _batch(arr, dtype, size):
        """[h, w] or [n, h, w] of `dtype`, rows and images possibly strided (pixels of a row contiguous) -> (array [n, h, w], single)"""
        arr = np.asarray(arr)
        single = arr.ndim == 2
        a = arr[None] if single else arr
        assert a.dtype == dtype and a.ndim == 3 and a.shape[1:] == (size[1], size[0]), (a.dtype, a.shape)
        if a.strides[2] != a.itemsize or a.strides[1] < a.shape[2] * a.itemsize or (len(a) > 1 and a.strides[0] < a.strides[1] * a.shape[1]):
            a = np.ascontiguousarray(a)
        return a, single

    def depth(self, arr, out=None):
        """arr: uint16 [h_s, w_s] or [n, h_s, w_s] -> (uint16 [n, h_d, w_d], index int32 [n, h_d, w_d], counters int64 [n, 8]); out: where the
        depth images go (strided rows allowed; only its pixels are written)"""
        a, single = self._batch(arr, np.uint16, self.src_size)
        n = len(a)
        if out is None:
            o = np.zeros((n, self.dst_size[1], self.dst_size[0]), dtype=np.uint16)
        else:
            o = out[None] if out.ndim == 2 else out
            assert o.dtype == np.uint16 and o.shape == (n, self.dst_size[1], self.dst_size[0]) and o.strides[2] == 2 and o.flags.writeable
        idx = np.zeros((n, self.dst_size[1], self.dst_size[0]), dtype=np.int32); cnt = np.zeros((n, 8), dtype=np.int64)
        _check(self.L.vc_register_depth(self.h, n, C.c_void_p(a.ctypes.data), int(a.strides[1]), C.c_longlong(a.strides[0]), C.c_void_p(o.ctypes.data), int(o.strides[1]),
                                        C.c_longlong(o.strides[0]), C.c_void_p(idx.ctypes.data), C.c_void_p(cnt.ctypes.data)), "register_depth")
        return (o[0], idx[0], cnt[0]) if single else (o, idx, cnt)

    def depth_device(self, n, d_src, src_pitch, src_stride, d_dst, dst_pitch, dst_stride, d_index=None, d_counters=None):
        """Device pointers (integers), enqueued on stream() without synchronisation (vc_register_depth_device)."""
        vp = lambda x: None if x is None else C.c_void_p(int(x))      # noqa: E731
        _check(self.L.vc_register_depth_device(self.h, int(n), vp(d_src), int(src_pitch), C.c_longlong(src_stride), vp(d_dst), int(dst_pitch), C.c_longlong(dst_stride),
                                               vp(d_index), vp(d_counters)), "register_depth_device")

    def stream(self): return self.L.vc_register_stream(self.h)

    def color(self, depth, images, occl_tol=0.0, fill=0):
        """depth: uint16 [n, h_s, w_s] of S; images: uint8 [n, h_d, w_d] of D -> (uint8 [n, h_s, w_s], visible [n, h_s, w_s] bool)"""
        a, single = self._batch(depth, np.uint16, self.src_size)
        c, _ = self._batch(images, np.uint8, self.dst_size)
        n = len(a)
        assert len(c) == n
        o = np.zeros((n, self.src_size[1], self.src_size[0]), dtype=np.uint8); m = np.zeros_like(o)
        ll = C.c_longlong
        _check(self.L.vc_register_color(self.h, n, C.c_void_p(a.ctypes.data), int(a.strides[1]), ll(a.strides[0]), C.c_void_p(c.ctypes.data), int(c.strides[1]),
                                        ll(c.strides[0]), C.c_double(occl_tol), int(fill), C.c_void_p(o.ctypes.data), int(o.strides[1]), ll(o.strides[0]),
                                        C.c_void_p(m.ctypes.data)), "register_color")
        return (o[0], m[0].astype(bool)) if single else (o, m.astype(bool))

    def points(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 3)
        out = np.zeros_like(rows); valid = np.zeros(len(rows), dtype=np.uint8)
        _check(self.L.vc_register_points(self.h, len(rows), _d(rows), out.ctypes.data_as(C.c_void_p), valid.ctypes.data_as(C.c_void_p)), "register_points")
        return out, valid.astype(bool)

    def time(self, n_images=8, reps=20):
        """Average ms per launch: table build, clear + scatter + resolve of n_images device-resident images, gather, 65536 points."""
        out = np.zeros(4)
        _check(self.L.vc_time_register(self.h, int(n_images), int(reps), _d(out)), "time_register")
        return dict(tables=out[0], depth=out[1], gather=out[2], points=out[3])


class DepthCalibrator:
    """The range error of a depth camera measured against the calibration target, and its correction (include/vicalib_amd.h:
    vc_depthcal*).  cam is (model, params, (w, h), T_ck) of the depth camera; rect = (x0, y0, x1, y1) the board in the target plane;
    kind "z" or "range".  add(depth, T_wk) -> counters [n, 8]; expected(T_wk, depth=None) -> (y [n, h, w], rule [n, h, w]);
    sums() -> dict; fit(degree) -> dict; apply(depth, interp) -> (corrected, counters [n, 3])."""
    KINDS = Registrar.KINDS
    INTERPS = {"cell": 0, "bilinear": 1}

    def __init__(self, cam, rect, bins=(4, 3), unit=0.001, kind="z", v_ref=1000.0, min_cos=0.5, max_dev=100.0, device=0, _camera_of=None):
        self.L = load()
        self.h = C.c_void_p()
        kind = self.KINDS.get(kind, kind)
        tail = (C.c_double(unit), int(kind), _d(rect), int(bins[0]), int(bins[1]), C.c_double(v_ref), C.c_double(min_cos), C.c_double(max_dev), C.byref(self.h))
        if _camera_of is not None:
            cal, c = _camera_of
            _check(self.L.vc_depthcal_create_for_camera(cal.h, int(c), *tail), "depthcal_create_for_camera")
        else:
            m, K, size, T = cam
            K = np.ascontiguousarray(K, dtype=np.float64)
            _check(self.L.vc_depthcal_create(int(device), _model_id(m), _d(K), len(K), int(size[0]), int(size[1]), _d(T), *tail), "depthcal_create")
        g = self.get()
        self.size, self.bins = g["size"], g["bins"]
        self.cells = self.bins[0] * self.bins[1]

    @classmethod
    def for_camera(cls, cal, cam, rect, **kw):
        """For a camera of a ViCalibrator, with the model, parameters, size and pose it holds for it."""
        return cls(None, rect, _camera_of=(cal, cam), **kw)

    def close(self):
        if getattr(self, "h", None):
            self.L.vc_depthcal_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def get(self):
        """-> dict(size, bins, unit, kind, rect, v_ref, min_cos, max_dev, R_ck, t_ck)"""
        size = (C.c_int * 2)(); bins = (C.c_int * 2)(); unit = C.c_double(0); kind = C.c_int(0); rect = np.zeros(4)
        v_ref = C.c_double(0); min_cos = C.c_double(0); max_dev = C.c_double(0); R = np.zeros((3, 3)); t = np.zeros(3)
        _check(self.L.vc_depthcal_get(self.h, size, bins, C.byref(unit), C.byref(kind), _d(rect), C.byref(v_ref), C.byref(min_cos), C.byref(max_dev), _d(R), _d(t)),
               "depthcal_get")
        return dict(size=(size[0], size[1]), bins=(bins[0], bins[1]), unit=unit.value, kind=kind.value, rect=rect, v_ref=v_ref.value, min_cos=min_cos.value,
                    max_dev=max_dev.value, R_ck=R, t_ck=t)

    def clear(self):
        _check(self.L.vc_depthcal_clear(self.h), "depthcal_clear")

    def _images(self, arr):
        a, _ = Registrar._batch(arr, np.uint16, self.size)
        return a

    @staticmethod
    def _poses(T_wk, n):
        T = np.ascontiguousarray(T_wk, dtype=np.float64).reshape(-1, 7)
        assert len(T) == n, (len(T), n)
        return T

    def add(self, depth, T_wk):
        """depth: uint16 [h, w] or [n, h, w] (strided rows and images allowed); T_wk: [n, 7] -> counters int64 [n, 8]"""
        a = self._images(depth)
        n = len(a)
        T = self._poses(T_wk, n)
        cnt = np.zeros((n, 8), dtype=np.int64)
        _check(self.L.vc_depthcal_add(self.h, n, C.c_void_p(a.ctypes.data), int(a.strides[1]), C.c_longlong(a.strides[0]), _d(T), C.c_void_p(cnt.ctypes.data)), "depthcal_add")
        return cnt

    def expected(self, T_wk, depth=None):
        """-> (y float64 [n, h, w], rule uint8 [n, h, w]); without depth rules 0 and 6 are not applied"""
        T = np.ascontiguousarray(T_wk, dtype=np.float64).reshape(-1, 7)
        n = len(T)
        y = np.zeros((n, self.size[1], self.size[0])); rule = np.zeros(y.shape, dtype=np.uint8)
        if depth is None:
            ptr, pitch, stride = None, 0, 0
        else:
            a = self._images(depth)
            assert len(a) == n
            ptr, pitch, stride = C.c_void_p(a.ctypes.data), int(a.strides[1]), int(a.strides[0])
        _check(self.L.vc_depthcal_expected(self.h, n, _d(T), ptr, pitch, C.c_longlong(stride), C.c_void_p(y.ctypes.data), C.c_void_p(rule.ctypes.data)), "depthcal_expected")
        return y, rule

    def sums(self):
        """-> dict(sums [cells, 9], totals [9], counters [8], n_frames)"""
        s = np.zeros((self.cells, 9)); tot = np.zeros(9); cnt = np.zeros(8, dtype=np.int64); nf = C.c_longlong(0)
        _check(self.L.vc_depthcal_sums(self.h, C.c_void_p(s.ctypes.data), C.c_void_p(tot.ctypes.data), C.c_void_p(cnt.ctypes.data), C.byref(nf)), "depthcal_sums")
        return dict(sums=s, totals=tot, counters=cnt, n_frames=nf.value)

    def fit(self, degree=2, min_count=50, min_spread=0.02):
        _check(self.L.vc_depthcal_fit(self.h, int(degree), int(min_count), C.c_double(min_spread)), "depthcal_fit")
        return self.get_fit()

    def get_fit(self):
        """-> dict(c [3], a, b, status [cells], rms [3], degree)"""
        c = np.zeros(3); a = np.zeros(self.cells); b = np.zeros(self.cells); st = np.zeros(self.cells, dtype=np.int32); rms = np.zeros(3); deg = C.c_int(0)
        _check(self.L.vc_depthcal_get_fit(self.h, C.c_void_p(c.ctypes.data), C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), C.c_void_p(st.ctypes.data),
                                          C.c_void_p(rms.ctypes.data), C.byref(deg)), "depthcal_get_fit")
        return dict(c=c, a=a, b=b, status=st, rms=rms, degree=deg.value)

    def set_fit(self, degree, c, a, b):
        a = np.ascontiguousarray(a, dtype=np.float64).ravel(); b = np.ascontiguousarray(b, dtype=np.float64).ravel()
        assert len(a) == self.cells and len(b) == self.cells and len(c) == 3
        _check(self.L.vc_depthcal_set_fit(self.h, int(degree), _d(c), _d(a), _d(b)), "depthcal_set_fit")

    def apply(self, depth, interp="cell", out=None):
        """depth: uint16 [h, w] or [n, h, w] -> (corrected uint16 [n, h, w], counters int64 [n, 3]: zeros in, corrected, out of range); out: where
        the images go (strided rows allowed, `depth` itself included; only its pixels are written)"""
        a = self._images(depth)
        n = len(a)
        if out is None:
            o = np.zeros((n, self.size[1], self.size[0]), dtype=np.uint16)
        else:
            o = out[None] if out.ndim == 2 else out
            assert o.dtype == np.uint16 and o.shape == a.shape and o.strides[2] == 2 and o.flags.writeable
        cnt = np.zeros((n, 3), dtype=np.int64)
        _check(self.L.vc_depthcal_apply(self.h, n, C.c_void_p(a.ctypes.data), int(a.strides[1]), C.c_longlong(a.strides[0]), C.c_void_p(o.ctypes.data), int(o.strides[1]),
                                        C.c_longlong(o.strides[0]), int(self.INTERPS.get(interp, interp)), C.c_void_p(cnt.ctypes.data)), "depthcal_apply")
        return o, cnt

    def time(self, n_images=8, reps=20):
        """Average ms per launch: table build, accumulate + fold of n_images device-resident images, apply."""
        out = np.zeros(3)
        _check(self.L.vc_time_depthcal(self.h, int(n_images), int(reps), _d(out)), "time_depthcal")
        return dict(tables=out[0], accumulate=out[1], apply=out[2])


def allan_factors(n_used, per_decade=20, max_fraction=1.0 / 9.0):
    """The averaging factors of an Allan deviation over n_used samples and IEEE Std 952's relative standard error of every point
    (vc_allan_factors; host only) -> (m int32 [n_m], rel_err [n_m])."""
    L = load()
    n_m = C.c_int(0)
    _check(L.vc_allan_factors(int(n_used), int(per_decade), C.c_double(max_fraction), 0, None, None, C.byref(n_m)), "allan_factors")
    m = np.zeros(n_m.value, dtype=np.int32); e = np.zeros(n_m.value)
    _check(L.vc_allan_factors(int(n_used), int(per_decade), C.c_double(max_fraction), len(m), C.c_void_p(m.ctypes.data), C.c_void_p(e.ctypes.data), C.byref(n_m)),
           "allan_factors")
    return m, e


def allan_fit(tau, avar, rel_err):
    """White noise N, bias instability B and rate random walk K of one Allan variance curve (vc_allan_fit; host only) ->
    dict(N, B, K, mask, rms_log, n_points, status); status 1: fewer than three usable points, 2: no feasible subset of the terms."""
    tau = np.ascontiguousarray(tau, dtype=np.float64).reshape(-1); avar = np.ascontiguousarray(avar, dtype=np.float64).reshape(-1)
    e = np.ascontiguousarray(rel_err, dtype=np.float64).reshape(-1)
    if not (len(tau) == len(avar) == len(e)) or len(tau) < 1:
        raise VicalibError("allan_fit: tau, avar and rel_err need the same length, at least 1")
    out = np.zeros(5); mask = C.c_int(0)
    st = _check(load().vc_allan_fit(len(tau), _d(tau), _d(avar), _d(e), C.c_void_p(out.ctypes.data), C.byref(mask)), "allan_fit")
    return dict(N=out[0], B=out[1], K=out[2], rms_log=out[3], n_points=int(out[4]), mask=mask.value, status=st)


class AllanAnalyzer:
    """The noise of an IMU from a log recorded at rest (include/vicalib_amd.h: vc_allan*): the log's means and prefix sums live on the device;
    run(m) -> (avar [6, n_m], terms [n_m]) over the range in use; static(window, gyro_thr, accel_thr) finds the longest quiet stretch and makes
    it the range; set_range(first, count).  gyro, accel: [n, 3]; time: [n], strictly increasing.  Channels gx gy gz ax ay az."""

    def __init__(self, gyro, accel, time, device=0):
        self.L = load()
        self.h = C.c_void_p()
        g = np.ascontiguousarray(gyro, dtype=np.float64); a = np.ascontiguousarray(accel, dtype=np.float64); t = np.ascontiguousarray(time, dtype=np.float64).reshape(-1)
        if g.ndim != 2 or g.shape[1] != 3 or a.shape != g.shape or len(t) != len(g):
            raise VicalibError("AllanAnalyzer: gyro and accel need the shape [n, 3], time the length n")
        _check(self.L.vc_allan_create(int(device), len(t), _d(g), _d(a), _d(t), C.byref(self.h)), "allan_create")
        self.n = len(t)

    def close(self):
        if getattr(self, "h", None):
            self.L.vc_allan_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def get(self):
        """-> dict(n, tau0, dt_min, dt_max, means [6], irregular, range (first, count))"""
        n = C.c_int(0); tau0 = C.c_double(0); lo = C.c_double(0); hi = C.c_double(0); means = np.zeros(6); irr = C.c_longlong(0); rng = (C.c_int * 2)()
        _check(self.L.vc_allan_get(self.h, C.byref(n), C.byref(tau0), C.byref(lo), C.byref(hi), C.c_void_p(means.ctypes.data), C.byref(irr), rng), "allan_get")
        return dict(n=n.value, tau0=tau0.value, dt_min=lo.value, dt_max=hi.value, means=means, irregular=irr.value, range=(rng[0], rng[1]))

    def set_range(self, first, count):
        _check(self.L.vc_allan_set_range(self.h, int(first), int(count)), "allan_set_range")

    def static(self, window, gyro_thr=0.0, accel_thr=0.0):
        """-> (status, first, count, n_quiet); status 1: no window start is quiet, the range stays"""
        rng = (C.c_int * 2)(); nq = C.c_int(0)
        st = _check(self.L.vc_allan_static(self.h, int(window), C.c_double(gyro_thr), C.c_double(accel_thr), rng, C.byref(nq)), "allan_static")
        return st, rng[0], rng[1], nq.value

    @staticmethod
    def _factors(m):
        m = np.ascontiguousarray(m, dtype=np.int32).reshape(-1)
        if len(m) < 1:
            raise VicalibError("AllanAnalyzer: at least one averaging factor is needed")
        return m

    def run(self, m):
        m = self._factors(m)
        avar = np.zeros((6, len(m))); terms = np.zeros(len(m), dtype=np.int32)
        _check(self.L.vc_allan_run(self.h, len(m), C.c_void_p(m.ctypes.data), C.c_void_p(avar.ctypes.data), C.c_void_p(terms.ctypes.data)), "allan_run")
        return avar, terms

    def time(self, m, reps=10):
        """mean ms of one launch set, `reps` back to back between HIP events: dict(scan, sweep)"""
        m = self._factors(m)
        out = np.zeros(2)
        _check(self.L.vc_time_allan(self.h, len(m), C.c_void_p(m.ctypes.data), int(reps), C.c_void_p(out.ctypes.data)), "time_allan")
        return dict(scan=out[0], sweep=out[1])
