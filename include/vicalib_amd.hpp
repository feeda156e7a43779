// vicalib_amd.hpp -- C++ face of libvicalib_amd.so: the public surface of
// visual_inertial_calibration::ViCalibrator (reference include/vicalib/vicalibrator.h:119-544) with the same
// member names, argument order and meaning, over the C ABI of vicalib_amd.h.  Header-only, no dependencies
// (the reference's Sophus/Calibu/Eigen types are replaced by plain aggregates with the same memory layout:
// Se3 = Sophus::SE3d::data() = [qx qy qz qw tx ty tz]).  INTEGRATION.md shows the variant that keeps the
// Calibu / Sophus types for a build inside the vicalib tree.
#pragma once
#include <vicalib_amd.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <stdexcept>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace visual_inertial_calibration {

struct Se3 {
  std::array<double, 7> v{{0, 0, 0, 1, 0, 0, 0}};
  double* data() { return v.data(); }
  const double* data() const { return v.data(); }
};

// CameraAndPose (vicalibrator.h:65-73): the calibu camera becomes (model id, parameter vector, image size)
struct CameraAndPose {
  int model = VC_MODEL_POLY3;
  std::vector<double> params;
  int width = 0, height = 0;
  Se3 T_ck;
};
struct VicalibFrame {          // vicalibrator.h:76-97
  Se3 t_wp_;
  std::array<double, 3> v_w_{{0, 0, 0}};
  double time = 0;
};

// The reference CHECK-aborts on misuse (bad index, setter while running, :333-:391); the wrapper throws instead of
// dropping the status code.
inline int vc_checked(int rc, const char* what) {
  if (rc < 0) throw std::runtime_error(std::string("vicalib_amd: ") + what + " failed (status " + std::to_string(rc) + ")");
  return rc;
}

// The focal-length seed of every camera from its views of the planar target (vc_seed_focal_batch; on the device, no handle).
struct SeedFocalResult {
  std::vector<double> view_H, view_rows, view_f, view_fit_px;      // x 9, x 4 (c1 d1 c2 d2), x 1, x 1 per view; NaN where the view was refused
  std::vector<int> view_used, view_status;
  std::vector<double> cam_f;                                       // NaN where the camera was refused
  std::vector<int> cam_views, cam_status;
};
inline SeedFocalResult SeedFocalBatch(int device, const std::vector<int>& view_cam, const std::vector<double>& cam_pp, const std::vector<double>& cam_radius,
                                      const std::vector<int>& view_off, const std::vector<double>& p_w, const std::vector<double>& p_c, int min_corners = 4,
                                      double max_fit_px = 0.0, double min_tilt_deg = 5.0) {
  const size_t nv = view_cam.size(), nc = cam_radius.size();
  if (view_off.size() != nv + 1 || cam_pp.size() != 2 * nc) throw std::runtime_error("vicalib_amd: SeedFocalBatch: array sizes disagree");
  const double nan = std::nan("");
  SeedFocalResult r;
  r.view_H.assign(9 * nv + 1, nan); r.view_rows.assign(4 * nv + 1, nan); r.view_f.assign(nv + 1, nan); r.view_fit_px.assign(nv + 1, nan);
  r.view_used.assign(nv + 1, 0); r.view_status.assign(nv + 1, -1); r.cam_f.assign(nc + 1, nan); r.cam_views.assign(nc + 1, 0); r.cam_status.assign(nc + 1, -1);
  const double none[3] = {0, 0, 0};
  vc_checked(vc_seed_focal_batch(device, (int)nv, nv ? view_cam.data() : r.view_used.data(), (int)nc, cam_pp.data(), cam_radius.data(), view_off.data(),
                                 p_w.empty() ? none : p_w.data(), p_c.empty() ? none : p_c.data(), min_corners, max_fit_px, min_tilt_deg, r.view_H.data(),
                                 r.view_rows.data(), r.view_f.data(), r.view_fit_px.data(), r.view_used.data(), r.view_status.data(), r.cam_f.data(),
                                 r.cam_views.data(), r.cam_status.data()), "SeedFocalBatch");
  r.view_H.resize(9 * nv); r.view_rows.resize(4 * nv); r.view_f.resize(nv); r.view_fit_px.resize(nv); r.view_used.resize(nv); r.view_status.resize(nv);
  r.cam_f.resize(nc); r.cam_views.resize(nc); r.cam_status.resize(nc);
  return r;
}

// The predicted bias of every dot's measured centre (vc_dot_bias_batch; on the device, no handle): view v has the camera view_model / view_K
// (x 10) and the pose view_T_cw (x 7, target into camera) and owns observations view_off[v] .. view_off[v+1]-1 of p_w (x 3) / radius (metres).
struct DotBiasResult {
  std::vector<double> bias, radius_px;      // x 2, x 1 per observation; NaN where the observation was refused
  std::vector<int> status;
};
inline DotBiasResult DotBiasBatch(int device, const std::vector<int>& view_model, const std::vector<double>& view_K, const std::vector<double>& view_T_cw,
                                  const std::vector<int>& view_off, const std::vector<double>& p_w, const std::vector<double>& radius) {
  const size_t nv = view_model.size(), n = radius.size();
  if (view_K.size() != 10 * nv || view_T_cw.size() != 7 * nv || view_off.size() != nv + 1 || p_w.size() != 3 * n || view_off.front() != 0 || (size_t)view_off.back() != n)
    throw std::runtime_error("vicalib_amd: DotBiasBatch: array sizes disagree");
  const double nan = std::nan("");
  DotBiasResult r;
  r.bias.assign(2 * n + 1, nan); r.radius_px.assign(n + 1, nan); r.status.assign(n + 1, -1);
  const double none[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  vc_checked(vc_dot_bias_batch(device, (int)nv, nv ? view_model.data() : r.status.data(), nv ? view_K.data() : none, nv ? view_T_cw.data() : none, view_off.data(),
                               n ? p_w.data() : none, n ? radius.data() : none, r.bias.data(), r.radius_px.data(), r.status.data()), "DotBiasBatch");
  r.bias.resize(2 * n); r.radius_px.resize(n); r.status.resize(n);
  return r;
}

// One Gauss-Newton step on the target's points with the frame poses and the shared camera columns marginalised (vc_target_refine_batch; on the
// device, no handle).  The rig as for vc_selector_create (model, params x 10, T_ck x 7, flags per camera), poses x 7 per frame, tile t = corners
// tile_off[t] .. tile_off[t+1]-1 of point_id / p_c (x 2) of (tile_frame[t], tile_cam[t]); points and nominal x 3 per target point.
struct TargetRefineResult {
  std::vector<double> refined;                        // x 3 per point; a singular result returns `points`
  std::vector<int> point_status, point_corners;       // 0 refined, 1 no usable corner (its row of refined is its row of points)
  std::vector<int> frame_status;                      // x 3 per frame: status, corners, behind
  int gauge_rank = 0, status = -1;                    // status: 0 ok, 1 singular
  double cost = 0, predicted_decrease = 0;
};
inline TargetRefineResult TargetRefineBatch(int device, const std::vector<int>& model, const std::vector<double>& params, const std::vector<double>& T_ck,
                                            const std::vector<int>& cam_flags, const std::vector<double>& T_wk, const std::vector<int>& tile_frame,
                                            const std::vector<int>& tile_cam, const std::vector<long long>& tile_off, const std::vector<int>& point_id,
                                            const std::vector<double>& p_c, const std::vector<double>& points, const std::vector<double>& nominal, double lambda) {
  const size_t nc = model.size(), nf = T_wk.size() / 7, nt = tile_frame.size(), np = points.size() / 3;
  if (params.size() != 10 * nc || T_ck.size() != 7 * nc || cam_flags.size() != nc || T_wk.size() != 7 * nf || tile_cam.size() != nt || tile_off.size() != nt + 1 ||
      p_c.size() != 2 * point_id.size() || nominal.size() != points.size() || points.size() != 3 * np || (size_t)tile_off.back() > point_id.size())
    throw std::runtime_error("vicalib_amd: TargetRefineBatch: array sizes disagree");
  TargetRefineResult r;
  r.refined = points; r.refined.resize(3 * np + 1);
  r.point_status.assign(np + 1, -1); r.point_corners.assign(np + 1, 0); r.frame_status.assign(3 * nf + 1, 0);
  const int none_i[1] = {0};
  const double none_d[2] = {0, 0};
  vc_checked(vc_target_refine_batch(device, (int)nc, model.data(), params.data(), T_ck.data(), cam_flags.data(), (int)nf, T_wk.data(), (int)nt,
                                    nt ? tile_frame.data() : none_i, nt ? tile_cam.data() : none_i, tile_off.data(), point_id.empty() ? none_i : point_id.data(),
                                    p_c.empty() ? none_d : p_c.data(), points.data(), nominal.data(), (int)np, lambda, r.refined.data(), r.point_status.data(),
                                    r.point_corners.data(), r.frame_status.data(), &r.gauge_rank, &r.status, &r.cost, &r.predicted_decrease), "TargetRefineBatch");
  r.refined.resize(3 * np); r.point_status.resize(np); r.point_corners.resize(np); r.frame_status.resize(3 * nf);
  return r;
}

// The inertial seed (vc_seed_imu, vc_seed_imu_sweep; on the device, no handle): the rotation camera <- IMU, the time offset, the gyro bias and the
// direction of gravity from the frames' camera rotations (frame_q_wc: n x 4, [x y z w]; frame_ok: 0 = no rotation) and the IMU log.
struct SeedImuResult {
  int status = -1, count = 0;                   // 0 ok, 1 too few intervals, 2 the minimum on the edge of the range, 3 not finite
  double time_offset = 0, R_ck[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, gyro_bias[3] = {0, 0, 0}, g_dir[2] = {0, 0}, rms = 0, signal = 0;      // filled with status 0
  std::vector<double> coarse_lags, coarse_J;
};
struct SeedImuSweepResult { std::vector<double> J, R, bias, moments; std::vector<int> count; };      // per lag: 1, 9, 3, 18, 1
inline SeedImuSweepResult SeedImuSweep(int device, const std::vector<double>& frame_t, const std::vector<double>& frame_q_wc, const std::vector<unsigned char>& frame_ok,
                                       const std::vector<double>& imu_t, const std::vector<double>& gyro, const std::vector<double>& accel,
                                       const std::vector<double>& lags, double max_gap_s = 0.5, int min_intervals = 10) {
  const size_t nf = frame_t.size(), ns = imu_t.size(), nl = lags.size();
  if (frame_q_wc.size() != 4 * nf || frame_ok.size() != nf || gyro.size() != 3 * ns || accel.size() != 3 * ns) throw std::runtime_error("vicalib_amd: SeedImuSweep: array sizes disagree");
  SeedImuSweepResult r;
  r.J.resize(nl); r.R.resize(9 * nl); r.bias.resize(3 * nl); r.moments.resize(18 * nl); r.count.resize(nl);
  vc_checked(vc_seed_imu_sweep(device, (int)nf, frame_t.data(), frame_q_wc.data(), frame_ok.data(), (int)ns, imu_t.data(), gyro.data(), accel.data(), max_gap_s,
                               min_intervals, (int)nl, lags.data(), r.J.data(), r.R.data(), r.bias.data(), r.count.data(), r.moments.data()), "SeedImuSweep");
  return r;
}
inline SeedImuResult SeedImu(int device, const std::vector<double>& frame_t, const std::vector<double>& frame_q_wc, const std::vector<unsigned char>& frame_ok,
                             const std::vector<double>& imu_t, const std::vector<double>& gyro, const std::vector<double>& accel, double range_s = 0.5,
                             double step_s = 0.0, int fine = 8, double max_gap_s = 0.5, int min_intervals = 10) {
  const size_t nf = frame_t.size(), ns = imu_t.size();
  if (frame_q_wc.size() != 4 * nf || frame_ok.size() != nf || gyro.size() != 3 * ns || accel.size() != 3 * ns) throw std::runtime_error("vicalib_amd: SeedImu: array sizes disagree");
  SeedImuResult r;
  int n_coarse = 0;
  for (int pass = 0; pass < 2; ++pass) {                                     // (the coarse curve is caller-sized: a longer one is fetched by a second call)
    r.coarse_lags.assign((size_t)(n_coarse > 4096 ? n_coarse : 4096), 0.0); r.coarse_J.assign(r.coarse_lags.size(), 0.0);
    vc_checked(vc_seed_imu(device, (int)nf, frame_t.data(), frame_q_wc.data(), frame_ok.data(), (int)ns, imu_t.data(), gyro.data(), accel.data(), max_gap_s,
                           min_intervals, range_s, step_s, fine, &r.time_offset, r.R_ck, r.gyro_bias, r.g_dir, &r.rms, &r.signal, &r.count, &r.status,
                           (int)r.coarse_lags.size(), r.coarse_lags.data(), r.coarse_J.data(), &n_coarse), "SeedImu");
    if ((size_t)n_coarse <= r.coarse_lags.size()) break;
  }
  r.coarse_lags.resize((size_t)n_coarse); r.coarse_J.resize((size_t)n_coarse);
  return r;
}

// The rig seed: every camera's pose relative to camera 0 from the views it shares (vc_seed_rig; on the device, no handle).  view_ok
// [n_frames x n_cams], view_T_cw [n_frames x n_cams x 7]; a refused pair or a camera not reached keeps the fill (NaN poses, -1 counts).
struct SeedRigResult {
  std::vector<double> pair_T_ab, pair_rms_deg, pair_rms_m, cam_T_c0;      // per pair 7, 1, 1; per camera 7
  std::vector<int> pair_shared, pair_support, pair_winner, pair_status, cam_parent, cam_status;
};
inline SeedRigResult SeedRig(int device, int n_cams, const std::vector<unsigned char>& view_ok, const std::vector<double>& view_T_cw, double tol_deg = 3.0,
                             int min_support = 3) {
  if (n_cams < 1 || view_ok.size() % (size_t)n_cams != 0 || view_T_cw.size() != 7 * view_ok.size()) throw std::runtime_error("vicalib_amd: SeedRig: array sizes disagree");
  const size_t nf = view_ok.size() / (size_t)n_cams, np = (size_t)n_cams * (n_cams - 1) / 2, pad = np ? np : 1;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  SeedRigResult r;
  r.pair_T_ab.assign(7 * pad, nan); r.pair_rms_deg.assign(pad, nan); r.pair_rms_m.assign(pad, nan); r.cam_T_c0.assign(7 * (size_t)n_cams, nan);
  r.pair_shared.assign(pad, 0); r.pair_support.assign(pad, -1); r.pair_winner.assign(pad, -1); r.pair_status.assign(pad, -1);
  r.cam_parent.assign((size_t)n_cams, -1); r.cam_status.assign((size_t)n_cams, -1);
  const unsigned char none = 0;
  vc_checked(vc_seed_rig(device, (int)nf, n_cams, nf ? view_ok.data() : &none, nf ? view_T_cw.data() : &nan, tol_deg, min_support, r.pair_T_ab.data(),
                         r.pair_shared.data(), r.pair_support.data(), r.pair_winner.data(), r.pair_rms_deg.data(), r.pair_rms_m.data(), r.pair_status.data(),
                         r.cam_T_c0.data(), r.cam_parent.data(), r.cam_status.data()), "SeedRig");
  r.pair_T_ab.resize(7 * np); r.pair_rms_deg.resize(np); r.pair_rms_m.resize(np);
  r.pair_shared.resize(np); r.pair_support.resize(np); r.pair_winner.resize(np); r.pair_status.resize(np);
  return r;
}

class ViCalibrator {
 public:
  explicit ViCalibrator(int device = 0) {
    const int rc = vc_create(&h_, device);
    if (rc != VC_OK) throw std::runtime_error(rc == VC_ERR_NO_DEVICE ? "vicalib_amd: no HIP device (there is no CPU fallback)" : "vicalib_amd: vc_create failed");
  }
  ~ViCalibrator() { vc_destroy(h_); }
  ViCalibrator(const ViCalibrator&) = delete;
  ViCalibrator& operator=(const ViCalibrator&) = delete;

  void Clear() { vc_checked(vc_clear(h_), "Clear"); }                                                         // :232
  int AddCamera(const CameraAndPose& c) {                                               // :332
    return vc_checked(vc_add_camera(h_, c.model, c.params.data(), (int)c.params.size(), c.width, c.height, c.T_ck.data()), "AddCamera");
  }
  void FixCameraIntrinsics(bool should_fix = true) { vc_checked(vc_fix_camera_intrinsics(h_, should_fix), "FixCameraIntrinsics"); }   // :346
  int AddFrame(const Se3& t_wk, double time) { return vc_checked(vc_add_frame(h_, t_wk.data(), time), "AddFrame"); }        // :355
  void SetFramePose(int frame, const Se3& t_wk) { vc_checked(vc_set_frame_pose(h_, frame, t_wk.data()), "SetFramePose"); }      // GetFrame(id)->t_wp_ = ...
  // AddObservation(frame, cam, p_w, p_c, time) :385 -- and its bulk form
  void AddObservation(size_t frame, size_t cam, const double p_w[3], const double p_c[2], double /*time*/) {
    vc_checked(vc_add_observations(h_, (int)frame, (int)cam, 1, p_w, p_c), "AddObservation");
  }
  void AddObservations(size_t frame, size_t cam, int n, const double* p_w, const double* p_c) {
    vc_checked(vc_add_observations(h_, (int)frame, (int)cam, n, p_w, p_c), "AddObservations");
  }
  bool AddImuMeasurements(const double gyro[3], const double accel[3], double time) {    // :370
    return vc_add_imu(h_, 1, gyro, accel, &time) == VC_OK;
  }
  int AddImuMeasurements(int n, const double* gyro, const double* accel, const double* time) { return vc_add_imu(h_, n, gyro, accel, time); }
  // robust branch of calibu::PosePnPRansac (iterations = 0: the reference's own call, vicalib-task.cc:323-325)
  void SetPnPRansac(int iterations, double tol_px) { vc_checked(vc_set_pnp_ransac(h_, iterations, tol_px), "SetPnPRansac"); }
  // the pose seeds (InitFramePosesPnP, HoldoutCompute without seeds) from the batched device PnP instead of the host routine
  void SetPnPDevice(bool on) { vc_checked(vc_set_pnp_device(h_, on ? 1 : 0), "SetPnPDevice"); }
  int InitFramePosesPnP() { int n = 0; vc_checked(vc_init_frame_poses_pnp(h_, &n), "InitFramePosesPnP"); return n; }      // vicalib-task.cc:335-348

  void SetOptimizationFlags(bool bias_active, bool inertial_active, bool rotation_only, bool optimize_imu_time_offset) {   // :252
    vc_checked(vc_set_optimization_flags(h_, bias_active, inertial_active, rotation_only, optimize_imu_time_offset), "SetOptimizationFlags");
  }
  void SetFunctionTolerance(double t) { vc_checked(vc_set_function_tolerance(h_, t), "SetFunctionTolerance"); }              // :277
  void SetSigmas(double gyro_sigma, double accel_sigma) { vc_checked(vc_set_sigmas(h_, gyro_sigma, accel_sigma), "SetSigmas"); }   // :290
  void SetTimeOffset(double t) { vc_checked(vc_set_time_offset(h_, t), "SetTimeOffset"); }                            // :296
  void SetBiases(const double b[6]) { vc_checked(vc_set_biases(h_, b), "SetBiases"); }                            // :301
  void SetScaleFactor(const double s[6]) { vc_checked(vc_set_scale_factor(h_, s), "SetScaleFactor"); }                 // :308
  // gflags the reference reads inside the class
  void SetMaxIters(int n) { vc_checked(vc_set_max_iters(h_, n), "SetMaxIters"); }
  void SetCalibrateImu(bool b) { vc_checked(vc_set_calibrate_imu(h_, b), "SetCalibrateImu"); }
  void SetRemoveOutliers(bool b, double threshold) { vc_checked(vc_set_remove_outliers(h_, b, threshold), "SetRemoveOutliers"); }

  void Start() { vc_checked(vc_start(h_), "Start"); }                                                         // :263
  bool IsRunning() { return vc_is_running(h_) > 0; }                                     // :314
  void Stop() { vc_checked(vc_stop(h_), "Stop"); }                                                           // :317
  int Solve() { return vc_solve(h_); }                                                   // Start() + join

  size_t NumFrames() { return (size_t)vc_num_frames(h_); }                               // :471
  size_t NumCameras() { return (size_t)vc_num_cameras(h_); }                             // :484
  double time_offset() { return vc_time_offset(h_); }                                    // :474
  double MeanSquaredError() { return vc_mean_squared_error(h_); }                        // :506
  unsigned GetNumIterations() { return vc_get_num_iterations(h_); }                      // :283
  std::vector<double> GetCameraProjRMSE() { std::vector<double> r(NumCameras()); vc_get_camera_proj_rmse(h_, r.data()); return r; }   // :160
  std::array<double, 6> GetBiases() { std::array<double, 6> b; vc_get_biases(h_, b.data()); return b; }              // :286
  std::array<double, 6> GetScaleFactor() { std::array<double, 6> s; vc_get_scale_factor(h_, s.data()); return s; }   // :306
  std::array<double, 2> GetGravity() { std::array<double, 2> g; vc_get_gravity(h_, g.data()); return g; }
  CameraAndPose GetCamera(size_t id) {                                                   // :492
    CameraAndPose c;
    c.params.resize(16);
    int n = 0;
    if (vc_get_camera(h_, (int)id, c.params.data(), &n, c.T_ck.data()) != VC_OK) throw std::out_of_range("GetCamera");
    c.params.resize(n);
    return c;
  }
  VicalibFrame GetFrame(size_t id) {                                                     // :477
    VicalibFrame f;
    if (vc_get_frame(h_, (int)id, f.t_wp_.data(), f.v_w_.data(), &f.time) != VC_OK) throw std::out_of_range("GetFrame");
    return f;
  }
  // imu_buffer() :487 (a copy: [gyro(3) accel(3) time] per measurement), GetIntegrationPoses(id) :508 (rows of 11: q t v time),
  // PrintResults() :536 (returned instead of logged)
  std::vector<std::array<double, 7>> imu_buffer() {
    const int n = vc_num_imu_measurements(h_);
    std::vector<double> g(3 * (size_t)std::max(n, 0)), a(g.size()), t((size_t)std::max(n, 0));
    std::vector<std::array<double, 7>> out((size_t)std::max(n, 0));
    if (n > 0) vc_checked(vc_get_imu_measurements(h_, g.data(), a.data(), t.data(), n), "imu_buffer");
    for (int i = 0; i < n; ++i) out[i] = {{g[3 * i], g[3 * i + 1], g[3 * i + 2], a[3 * i], a[3 * i + 1], a[3 * i + 2], t[i]}};
    return out;
  }
  std::vector<std::array<double, 11>> GetIntegrationPoses(unsigned id) {
    const int n = vc_checked(vc_get_integration_poses(h_, (int)id, nullptr, 0), "GetIntegrationPoses");      // the count first: all of them
    std::vector<std::array<double, 11>> out((size_t)std::max(n, 0));
    if (n > 0) vc_checked(vc_get_integration_poses(h_, (int)id, out[0].data(), n), "GetIntegrationPoses");
    return out;
  }
  std::string PrintResults() {
    // the length first (any number of cameras); a running Start() worker may lengthen the text between the two calls: slack + retry
    for (int attempt = 0; attempt < 8; ++attempt) {
      const int n = vc_checked(vc_print_results(h_, nullptr, 0), "PrintResults");
      std::string s((size_t)n + 65, '\0');
      if (vc_print_results(h_, &s[0], n + 65) >= 0) { s.resize(std::strlen(s.c_str())); return s; }
    }
    throw std::runtime_error("PrintResults: the text kept growing");
  }
  void WriteCameraModels(const std::string& filename) { vc_checked(vc_write_camera_models(h_, filename.c_str()), "WriteCameraModels"); }   // :208
  // GetSolutionCovariance(problem) :802-857: row-major n x n over the blocks named by covariance_names
  std::vector<double> GetSolutionCovariance(int* n_out = nullptr) {
    const int n = vc_solution_covariance_dim(h_);
    std::vector<double> cov(n > 0 ? (size_t)n * n : 0);
    int m = 0;
    if (n <= 0 || vc_get_solution_covariance(h_, cov.data(), n, &m) != VC_OK) cov.clear();
    if (n_out) *n_out = cov.empty() ? 0 : n;
    return cov;
  }
  std::string covariance_names() {
    std::string s(64 * 8 + 64, '\0');
    if (vc_get_solution_covariance_names(h_, &s[0], (int)s.size()) != VC_OK) return std::string();
    s.resize(s.find('\0'));
    return s;
  }
  // residual report (vc_report_*): compute once at the current state, then read
  struct ReportViews { std::vector<int> frame, camera, count, removed; std::vector<double> sum_sq, max_err; std::vector<long long> worst_corner; };
  void ReportCompute(int bins_x = 16, int bins_y = 12) { vc_checked(vc_report_compute(h_, bins_x, bins_y), "ReportCompute"); }
  void ReportCorners(long long first, long long n, double* r, int* frame, int* camera, unsigned char* flags) {
    vc_checked(vc_report_corners(h_, first, n, r, frame, camera, flags), "ReportCorners");
  }
  ReportViews GetReportViews() {
    const size_t n = (size_t)vc_checked(vc_report_num_views(h_), "ReportViews");
    ReportViews v;
    v.frame.resize(n); v.camera.resize(n); v.count.resize(n); v.removed.resize(n); v.sum_sq.resize(n); v.max_err.resize(n); v.worst_corner.resize(n);
    vc_checked(vc_report_views(h_, v.frame.data(), v.camera.data(), v.count.data(), v.removed.data(), v.sum_sq.data(), v.max_err.data(), v.worst_corner.data()), "ReportViews");
    return v;
  }
  std::vector<double> GetReportErrorMap(int camera, int bins_x, int bins_y) {      // bins_y x bins_x x 4, the bins of ReportCompute
    std::vector<double> m((size_t)bins_x * bins_y * 4);
    vc_checked(vc_report_error_map(h_, camera, m.data()), "ReportErrorMap");
    return m;
  }
  size_t NumReportImuBlocks() { return (size_t)vc_checked(vc_report_num_imu_blocks(h_), "ReportImu"); }
  void ReportImu(double* whitened, double* unwhitened, unsigned char* flags) { vc_checked(vc_report_imu(h_, whitened, unwhitened, flags), "ReportImu"); }
  // held-out scoring (vc_holdout_*): add the held-out views, compute at the current cameras, then read
  struct HoldoutFrames { std::vector<Se3> T_wk; std::vector<int> status, iterations, behind; std::vector<double> cost0, cost; };
  struct HoldoutViews { std::vector<int> frame, camera, count; std::vector<double> sum_sq, max_err; std::vector<long long> worst_corner; };
  struct HoldoutCameraRmse { std::vector<double> rmse; std::vector<long long> count; };
  void HoldoutClear() { vc_checked(vc_holdout_clear(h_), "HoldoutClear"); }
  void HoldoutAddTiles(int n_tiles, const int* tile_frame, const int* tile_cam, const long long* tile_off, const double* points, int n_points,
                       const int* point_id, const double* p_c) {
    vc_checked(vc_holdout_add_tiles(h_, n_tiles, tile_frame, tile_cam, tile_off, points, n_points, point_id, p_c), "HoldoutAddTiles");
  }
  void HoldoutCompute(const double* seeds = nullptr, int max_iters = 0) { vc_checked(vc_holdout_compute(h_, seeds, max_iters), "HoldoutCompute"); }
  HoldoutFrames GetHoldoutFrames() {
    const size_t n = (size_t)vc_checked(vc_holdout_num_frames(h_), "HoldoutFrames");
    HoldoutFrames f;
    std::vector<double> T(7 * n);
    f.T_wk.resize(n); f.status.resize(n); f.iterations.resize(n); f.behind.resize(n); f.cost0.resize(n); f.cost.resize(n);
    vc_checked(vc_holdout_frames(h_, T.data(), f.status.data(), f.iterations.data(), f.cost0.data(), f.cost.data(), f.behind.data()), "HoldoutFrames");
    for (size_t i = 0; i < n; ++i) std::memcpy(f.T_wk[i].data(), &T[7 * i], 56);
    return f;
  }
  HoldoutViews GetHoldoutViews() {
    const size_t n = (size_t)vc_checked(vc_holdout_num_views(h_), "HoldoutViews");
    HoldoutViews v;
    v.frame.resize(n); v.camera.resize(n); v.count.resize(n); v.sum_sq.resize(n); v.max_err.resize(n); v.worst_corner.resize(n);
    vc_checked(vc_holdout_views(h_, v.frame.data(), v.camera.data(), v.count.data(), v.sum_sq.data(), v.max_err.data(), v.worst_corner.data()), "HoldoutViews");
    return v;
  }
  long long NumHoldoutCorners() { const long long n = vc_holdout_num_corners(h_); vc_checked(n < 0 ? (int)n : 0, "HoldoutCorners"); return n; }
  void HoldoutCorners(long long first, long long n, double* r, int* frame, int* camera) {
    vc_checked(vc_holdout_corners(h_, first, n, r, frame, camera), "HoldoutCorners");
  }
  HoldoutCameraRmse GetHoldoutCameraRmse() {
    HoldoutCameraRmse c;
    c.rmse.resize(NumCameras()); c.count.resize(NumCameras());
    vc_checked(vc_holdout_camera_rmse(h_, c.rmse.data(), c.count.data()), "HoldoutCameraRmse");
    return c;
  }
  vc_calibrator* handle() { return h_; }

 private:
  vc_calibrator* h_ = nullptr;
};

// Using a calibration (vc_undistort*): a source camera's images and pixels mapped into a pinhole destination camera on the device.
struct LinearCamera { std::array<double, 4> fu_fv_u0_v0{{0, 0, 0, 0}}; int width = 0, height = 0; };
class Undistorter {
 public:
  // R_ds: row-major 3 x 3, source-camera rays -> destination-camera rays; nullptr = identity
  Undistorter(const CameraAndPose& src, const LinearCamera& dst, const double* R_ds = nullptr, int fill = 0, int device = 0) {
    vc_checked(vc_undistorter_create(device, src.model, src.params.data(), (int)src.params.size(), src.width, src.height, dst.fu_fv_u0_v0.data(), dst.width,
                                     dst.height, R_ds, fill, &u_), "Undistorter");
  }
  Undistorter(ViCalibrator& cal, int camera, const LinearCamera& dst, const double* R_ds = nullptr, int fill = 0) {
    vc_checked(vc_undistorter_create_for_camera(cal.handle(), camera, dst.fu_fv_u0_v0.data(), dst.width, dst.height, R_ds, fill, &u_), "Undistorter");
  }
  ~Undistorter() { vc_undistorter_destroy(u_); }
  Undistorter(const Undistorter&) = delete;
  Undistorter& operator=(const Undistorter&) = delete;
  // destination intrinsics for identity rotation: alpha = 0 every destination pixel has a source pixel, alpha = 1 every source pixel is kept
  static LinearCamera FitLinear(const CameraAndPose& src, int dst_width, int dst_height, double alpha = 0.0) {
    LinearCamera d; d.width = dst_width; d.height = dst_height;
    vc_checked(vc_undistort_fit_linear(src.model, src.params.data(), (int)src.params.size(), src.width, src.height, dst_width, dst_height, alpha, d.fu_fv_u0_v0.data()), "FitLinear");
    return d;
  }
  LinearCamera Linear() { LinearCamera d; int s[2] = {0, 0}; vc_checked(vc_undistort_get_linear(u_, d.fu_fv_u0_v0.data(), s), "Linear"); d.width = s[0]; d.height = s[1]; return d; }
  void Images(int n, const unsigned char* src, int src_pitch, long long src_stride, unsigned char* dst, int dst_pitch, long long dst_stride) {
    vc_checked(vc_undistort_images(u_, n, src, src_pitch, src_stride, dst, dst_pitch, dst_stride), "Images");
  }
  void ImagesDevice(int n, const unsigned char* d_src, int src_pitch, long long src_stride, unsigned char* d_dst, int dst_pitch, long long dst_stride) {
    vc_checked(vc_undistort_images_device(u_, n, d_src, src_pitch, src_stride, d_dst, dst_pitch, dst_stride), "ImagesDevice");
  }
  void* Stream() { return vc_undistort_stream(u_); }      // hipStream_t
  void Points(int n, const double* src_px, double* dst_px, unsigned char* valid = nullptr) { vc_checked(vc_undistort_points(u_, n, src_px, dst_px, valid), "Points"); }
  void Map(float* map, unsigned char* valid = nullptr) { vc_checked(vc_undistort_get_map(u_, map, valid), "Map"); }
  std::array<double, 3> Time(int n_images = 64, int reps = 20) { std::array<double, 3> ms{{0, 0, 0}}; vc_checked(vc_time_undistort(u_, n_images, reps, ms.data()), "Time"); return ms; }
  vc_undistorter* handle() { return u_; }

 private:
  vc_undistorter* u_ = nullptr;
};

// Using the calibration of a pair (vc_stereo_*, vc_rectif*): both cameras rotated into a common frame with one pinhole camera, image pairs
// remapped through the two sides' undistorters, and the stereo consistency check over matched corner pairs.
struct StereoCheck {                                   // vc_rectify_check: per pair, then per frame
  std::vector<double> pairs;                           // n x 6: dv, d, P (3), mean row
  std::vector<unsigned char> invalid;                  // n: 1 = the pair enters no sum
  std::vector<int> count, n_invalid;
  std::vector<double> sum_dv, sum_dv2, max_abs_dv, mean_z, rigid_rms;
  std::vector<long long> worst;
};
struct TileMatches { std::vector<int> frame; std::vector<long long> frame_off, pos_a, pos_b; };
class Rectifier {
 public:
  // dst.fu_fv_u0_v0 all zero: fitted at alpha (vc_stereo_fit_linear); dst.width / height are the destination size
  Rectifier(const CameraAndPose& a, const CameraAndPose& b, const LinearCamera& dst, double alpha = 0.0, int fill = 0, int device = 0) {
    vc_checked(vc_rectifier_create(device, a.model, a.params.data(), (int)a.params.size(), a.width, a.height, a.T_ck.data(), b.model, b.params.data(),
                                   (int)b.params.size(), b.width, b.height, b.T_ck.data(), Given(dst), dst.width, dst.height, alpha, fill, &r_), "Rectifier");
  }
  Rectifier(ViCalibrator& cal, int cam_a, int cam_b, const LinearCamera& dst, double alpha = 0.0, int fill = 0) {
    vc_checked(vc_rectifier_create_for_cameras(cal.handle(), cam_a, cam_b, Given(dst), dst.width, dst.height, alpha, fill, &r_), "Rectifier");
  }
  ~Rectifier() { vc_rectifier_destroy(r_); }
  Rectifier(const Rectifier&) = delete;
  Rectifier& operator=(const Rectifier&) = delete;
  // host code, no device: R_ds_a, R_ds_b (row-major) and the signed baseline
  static double Rotations(const Se3& T_ck_a, const Se3& T_ck_b, double R_ds_a[9], double R_ds_b[9]) {
    double b = 0.0;
    vc_checked(vc_stereo_rectify_rotations(T_ck_a.data(), T_ck_b.data(), R_ds_a, R_ds_b, &b), "Rotations");
    return b;
  }
  static LinearCamera FitLinear(const CameraAndPose& a, const double R_ds_a[9], const CameraAndPose& b, const double R_ds_b[9], int dst_width, int dst_height,
                                double alpha = 0.0) {
    LinearCamera d; d.width = dst_width; d.height = dst_height;
    vc_checked(vc_stereo_fit_linear(a.model, a.params.data(), (int)a.params.size(), a.width, a.height, R_ds_a, b.model, b.params.data(), (int)b.params.size(), b.width,
                                    b.height, R_ds_b, dst_width, dst_height, alpha, d.fu_fv_u0_v0.data()), "FitLinear");
    return d;
  }
  static TileMatches MatchTiles(int n_tiles, const int* tile_frame, const int* tile_cam, const long long* tile_off, const int* point_id, int cam_a, int cam_b) {
    TileMatches m; int nf = 0; long long n = 0;
    vc_checked(vc_match_tiles(n_tiles, tile_frame, tile_cam, tile_off, point_id, cam_a, cam_b, &nf, &n, nullptr, nullptr, nullptr, nullptr), "MatchTiles");
    m.frame.resize((size_t)nf); m.frame_off.resize((size_t)nf + 1); m.pos_a.resize((size_t)n + 1); m.pos_b.resize((size_t)n + 1);
    vc_checked(vc_match_tiles(n_tiles, tile_frame, tile_cam, tile_off, point_id, cam_a, cam_b, &nf, &n, m.frame.data(), m.frame_off.data(), m.pos_a.data(), m.pos_b.data()), "MatchTiles");
    m.pos_a.resize((size_t)n); m.pos_b.resize((size_t)n);
    return m;
  }
  vc_undistorter* Side(int side) { return vc_rectifier_side(r_, side); }      // borrowed
  LinearCamera Linear() { LinearCamera d; int s[2] = {0, 0}; vc_checked(vc_rectifier_get(r_, nullptr, nullptr, d.fu_fv_u0_v0.data(), s, nullptr, nullptr, nullptr), "Linear"); d.width = s[0]; d.height = s[1]; return d; }
  double Baseline() { double b = 0.0; vc_checked(vc_rectifier_get(r_, nullptr, nullptr, nullptr, nullptr, &b, nullptr, nullptr), "Baseline"); return b; }
  void RectifiedPoses(Se3* T_ck_rect_a, Se3* T_ck_rect_b) { vc_checked(vc_rectifier_get(r_, nullptr, nullptr, nullptr, nullptr, nullptr, T_ck_rect_a->data(), T_ck_rect_b->data()), "RectifiedPoses"); }
  void RotationMatrices(double R_ds_a[9], double R_ds_b[9]) { vc_checked(vc_rectifier_get(r_, R_ds_a, R_ds_b, nullptr, nullptr, nullptr, nullptr, nullptr), "RotationMatrices"); }
  void Pairs(int n, const unsigned char* src_a, int src_pitch_a, long long src_stride_a, const unsigned char* src_b, int src_pitch_b, long long src_stride_b,
             unsigned char* dst_a, int dst_pitch_a, long long dst_stride_a, unsigned char* dst_b, int dst_pitch_b, long long dst_stride_b) {
    vc_checked(vc_rectify_pairs(r_, n, src_a, src_pitch_a, src_stride_a, src_b, src_pitch_b, src_stride_b, dst_a, dst_pitch_a, dst_stride_a, dst_b, dst_pitch_b,
                                dst_stride_b), "Pairs");
  }
  // px_a, px_b: n x 2 distorted pixels, target: n x 3 or nullptr, n = frame_off.back()
  StereoCheck Check(const std::vector<long long>& frame_off, const double* px_a, const double* px_b, const double* target) {
    StereoCheck c;
    const size_t nf = frame_off.empty() ? 0 : frame_off.size() - 1, n = nf ? (size_t)frame_off.back() : 0;
    c.pairs.resize(6 * n + 1); c.invalid.resize(n + 1); c.count.resize(nf + 1); c.n_invalid.resize(nf + 1); c.worst.resize(nf + 1);
    for (std::vector<double>* v : {&c.sum_dv, &c.sum_dv2, &c.max_abs_dv, &c.mean_z, &c.rigid_rms}) v->resize(nf + 1);
    vc_checked(vc_rectify_check(r_, (int)nf, frame_off.data(), px_a, px_b, target, c.pairs.data(), c.invalid.data(), c.count.data(), c.n_invalid.data(), c.sum_dv.data(),
                                c.sum_dv2.data(), c.max_abs_dv.data(), c.worst.data(), c.mean_z.data(), c.rigid_rms.data()), "Check");
    c.pairs.resize(6 * n); c.invalid.resize(n); c.count.resize(nf); c.n_invalid.resize(nf); c.worst.resize(nf);
    for (std::vector<double>* v : {&c.sum_dv, &c.sum_dv2, &c.max_abs_dv, &c.mean_z, &c.rigid_rms}) v->resize(nf);
    return c;
  }
  double Time(int reps = 20) { double ms = 0.0; vc_checked(vc_time_rectify_check(r_, reps, &ms), "Time"); return ms; }
  vc_rectifier* handle() { return r_; }

 private:
  static const double* Given(const LinearCamera& d) { return (d.fu_fv_u0_v0[0] == 0.0 && d.fu_fv_u0_v0[1] == 0.0) ? nullptr : d.fu_fv_u0_v0.data(); }
  vc_rectifier* r_ = nullptr;
};

// Two calibrations of one camera compared in pixel space (vc_compar*): d = project(B, R unproject(A, q)) - q on a lattice over the image, at
// the implied rotation (fitted over the samples within fit_radius of the centre) or at a given one.
struct CompareFit { double R_ba[9]; int status = 0, iterations = 0, n_fit = 0, n_left_out = 0; double cost0 = 0, cost = 0; };
struct CompareSummary { long long count = 0, invalid = 0, worst = -1; double sum_du = 0, sum_dv = 0, sum_sq = 0, max_err = 0; };
struct CompareRings { std::vector<long long> count, invalid; std::vector<double> sum_sq, max_err; };
class Comparer {
 public:
  // a and b: model, params and size are read (the sizes must agree); the poses are not
  Comparer(const CameraAndPose& a, const CameraAndPose& b, int grid_x, int grid_y, int device = 0) : gx_(grid_x), gy_(grid_y) {
    if (a.width != b.width || a.height != b.height) throw std::runtime_error("vicalib_amd: Comparer: the two cameras' image sizes differ");
    vc_checked(vc_comparer_create(device, a.model, a.params.data(), (int)a.params.size(), b.model, b.params.data(), (int)b.params.size(), a.width, a.height, grid_x,
                                  grid_y, &c_), "Comparer");
  }
  Comparer(ViCalibrator& cal, int camera, const CameraAndPose& b, int grid_x, int grid_y) : gx_(grid_x), gy_(grid_y) {
    vc_checked(vc_comparer_create_for_camera(cal.handle(), camera, b.model, b.params.data(), (int)b.params.size(), grid_x, grid_y, &c_), "Comparer");
  }
  ~Comparer() { vc_comparer_destroy(c_); }
  Comparer(const Comparer&) = delete;
  Comparer& operator=(const Comparer&) = delete;
  // fit_radius <= 0: no fit, the difference at R_ba (nullptr = identity)
  CompareFit Run(double fit_radius = 0.5, int max_iters = 0, const double* R_ba = nullptr) {
    vc_checked(vc_compare_run(c_, fit_radius, max_iters, R_ba), "Run");
    CompareFit f;
    vc_checked(vc_compare_get_fit(c_, f.R_ba, &f.status, &f.iterations, &f.n_fit, &f.n_left_out, &f.cost0, &f.cost), "Run");
    return f;
  }
  // diff: gy x gx x 2 (a NaN pair at an invalid sample), flags: gy x gx
  void Map(std::vector<double>* diff, std::vector<unsigned char>* flags) {
    diff->resize(2 * (size_t)gx_ * gy_); flags->resize((size_t)gx_ * gy_);
    vc_checked(vc_compare_get_map(c_, diff->data(), flags->data()), "Map");
  }
  CompareSummary Summary() {
    CompareSummary s;
    vc_checked(vc_compare_summary(c_, &s.count, &s.invalid, &s.sum_du, &s.sum_dv, &s.sum_sq, &s.max_err, &s.worst), "Summary");
    return s;
  }
  CompareRings Rings(int n_rings = 8) {
    CompareRings r;
    const size_t n = n_rings > 0 ? (size_t)n_rings : 1;
    r.count.resize(n); r.invalid.resize(n); r.sum_sq.resize(n); r.max_err.resize(n);
    vc_checked(vc_compare_rings(c_, n_rings, r.count.data(), r.invalid.data(), r.sum_sq.data(), r.max_err.data()), "Rings");
    return r;
  }
  // host code, no device: [angle, distance] compensated by the implied rotations of cameras 0 and c, then [angle, distance] plain
  static std::array<double, 4> Extrinsics(const Se3& T_ck_a0, const Se3& T_ck_ac, const Se3& T_ck_b0, const Se3& T_ck_bc, const double* R_0, const double* R_c) {
    std::array<double, 4> out{{0, 0, 0, 0}};
    vc_checked(vc_compare_extrinsics(T_ck_a0.data(), T_ck_ac.data(), T_ck_b0.data(), T_ck_bc.data(), R_0, R_c, out.data()), "Extrinsics");
    return out;
  }
  std::array<double, 3> Time(int reps = 20) { std::array<double, 3> ms{{0, 0, 0}}; vc_checked(vc_time_compare(c_, reps, ms.data()), "Time"); return ms; }
  vc_comparer* handle() { return c_; }

 private:
  vc_comparer* c_ = nullptr;
  int gx_ = 0, gy_ = 0;
};

// A calibrated camera converted to another camera model (vc_convert*): the target's intrinsics fitted to the source's rays on a lattice over
// the image.  No change of extrinsics: the converted camera keeps the source's pose and size.
struct ConvertResult {
  std::vector<double> params;             // K_b
  int status = 0, iterations = 0, n_fit = 0, n_left_out = 0;
  double cost0 = 0, cost = 0, max_err = 0;
  long long worst = -1;
};
class Converter {
 public:
  // a: model, params and size are read; the pose is not
  Converter(const CameraAndPose& a, int model_b, int grid_x, int grid_y, int device = 0) {
    vc_checked(vc_converter_create(device, a.model, a.params.data(), (int)a.params.size(), a.width, a.height, model_b, grid_x, grid_y, &c_), "Converter");
  }
  Converter(ViCalibrator& cal, int camera, int model_b, int grid_x, int grid_y) {
    vc_checked(vc_converter_create_for_camera(cal.handle(), camera, model_b, grid_x, grid_y, &c_), "Converter");
  }
  ~Converter() { vc_converter_destroy(c_); }
  Converter(const Converter&) = delete;
  Converter& operator=(const Converter&) = delete;
  // start: nullptr = the source's [fu fv u0 v0] without distortion; free_mask: bit k set = K_b[k] is free, 0 = all
  ConvertResult Run(double fit_radius = 1.0, int max_iters = 0, const double* start = nullptr, unsigned int free_mask = 0) {
    vc_checked(vc_convert_run(c_, fit_radius, max_iters, start, free_mask), "Run");
    return Get();
  }
  ConvertResult Get() {
    ConvertResult r;
    int nk = 0;
    r.params.resize(10);
    vc_checked(vc_convert_get(c_, r.params.data(), &nk, &r.status, &r.iterations, &r.n_fit, &r.n_left_out, &r.cost0, &r.cost, &r.max_err, &r.worst), "Get");
    r.params.resize((size_t)nk);
    return r;
  }
  // a comparer of the source against the result on the same lattice; the caller destroys it (vc_comparer_destroy)
  vc_comparer* MakeComparer() { vc_comparer* cmp = nullptr; vc_checked(vc_convert_comparer(c_, &cmp), "MakeComparer"); return cmp; }
  std::array<double, 3> Time(int reps = 20) { std::array<double, 3> ms{{0, 0, 0}}; vc_checked(vc_time_convert(c_, reps, ms.data()), "Time"); return ms; }
  vc_converter* handle() { return c_; }

 private:
  vc_converter* c_ = nullptr;
};

// The projection uncertainty of one calibrated camera mapped over its image (vc_uncertainty*): per lattice sample the 2 x 2 covariance, in
// px^2, of the shift that a covariance of the intrinsics leaves after the rotation the extrinsics would absorb.  One camera on its own: the
// relative pose of a stereo pair is not in it.
struct UncertaintyFit { std::vector<double> M; double G[9]; int n_fit = 0; };      // M: 3 x nk, rad per unit of each parameter
struct UncertaintySummary { long long count = 0, invalid = 0, worst = -1; double sum_var = 0, max_lam = 0; };
struct UncertaintyRings { std::vector<long long> count, invalid; std::vector<double> sum_var, max_lam; };
class Uncertainty {
 public:
  // a: model, params and size are read; the pose is not.  Run needs a covariance.
  Uncertainty(const CameraAndPose& a, int grid_x, int grid_y, int device = 0) : nk_((int)a.params.size()), gx_(grid_x), gy_(grid_y) {
    vc_checked(vc_uncertainty_create(device, a.model, a.params.data(), (int)a.params.size(), a.width, a.height, grid_x, grid_y, &u_), "Uncertainty");
  }
  // the calibrator's camera with its block of the solution covariance at the current state
  Uncertainty(ViCalibrator& cal, int camera, int grid_x, int grid_y) : gx_(grid_x), gy_(grid_y) {
    vc_checked(vc_uncertainty_create_for_camera(cal.handle(), camera, grid_x, grid_y, &u_), "Uncertainty");
    nk_ = (int)cal.GetCamera(camera).params.size();
  }
  ~Uncertainty() { vc_uncertainty_destroy(u_); }
  Uncertainty(const Uncertainty&) = delete;
  Uncertainty& operator=(const Uncertainty&) = delete;
  // cov: nk x nk row-major, nullptr = the calibrator's; fit_radius <= 0: no compensation
  UncertaintyFit Run(const double* cov, double sigma_px, double fit_radius = 0.5) {
    vc_checked(vc_uncertainty_run(u_, cov, sigma_px, fit_radius), "Run");
    UncertaintyFit f;
    f.M.resize(3 * (size_t)nk_);
    vc_checked(vc_uncertainty_get_fit(u_, f.M.data(), f.G, &f.n_fit), "Run");
    return f;
  }
  // sigma: gy x gx x 3 = (s_uu, s_uv, s_vv), NaN at an invalid sample; flags: gy x gx
  void Map(std::vector<double>* sigma, std::vector<unsigned char>* flags) {
    sigma->resize(3 * (size_t)gx_ * gy_); flags->resize((size_t)gx_ * gy_);
    vc_checked(vc_uncertainty_get_map(u_, sigma->data(), flags->data()), "Map");
  }
  UncertaintySummary Summary() {
    UncertaintySummary s;
    vc_checked(vc_uncertainty_summary(u_, &s.count, &s.invalid, &s.sum_var, &s.max_lam, &s.worst), "Summary");
    return s;
  }
  UncertaintyRings Rings(int n_rings = 8) {
    UncertaintyRings r;
    const size_t n = n_rings > 0 ? (size_t)n_rings : 1;
    r.count.resize(n); r.invalid.resize(n); r.sum_var.resize(n); r.max_lam.resize(n);
    vc_checked(vc_uncertainty_rings(u_, n_rings, r.count.data(), r.invalid.data(), r.sum_var.data(), r.max_lam.data()), "Rings");
    return r;
  }
  std::array<double, 3> Time(int reps = 20) { std::array<double, 3> ms{{0, 0, 0}}; vc_checked(vc_time_uncertainty(u_, reps, ms.data()), "Time"); return ms; }
  vc_uncertainty* handle() { return u_; }

 private:
  vc_uncertainty* u_ = nullptr;
  int nk_ = 0, gx_ = 0, gy_ = 0;
};

// The row and depth uncertainty of a calibrated stereo pair mapped over its rectified image (vc_stereo_uncertainty*): per lattice sample and
// depth the variances of the row misalignment (px^2), the disparity (px^2) and the depth (m^2) that the joint covariance of the pair implies
// for pixels pushed through the rectifier's arithmetic.  The destination pinhole is held fixed.
struct StereoUncertaintySummary { long long count = 0, invalid = 0, worst = -1; double sum_var_dv = 0, sum_var_d = 0, sum_var_z = 0, max_var_dv = 0; };
class StereoUncertainty {
 public:
  // dst.fu_fv_u0_v0 all zero: fitted at alpha (vc_stereo_fit_linear); dst.width / height are the destination size.  Run needs a covariance.
  StereoUncertainty(const CameraAndPose& a, const CameraAndPose& b, const LinearCamera& dst, int grid_x, int grid_y, double alpha = 0.0, int device = 0)
      : gx_(grid_x), gy_(grid_y) {
    vc_checked(vc_stereo_uncertainty_create(device, a.model, a.params.data(), (int)a.params.size(), a.width, a.height, a.T_ck.data(), b.model, b.params.data(),
                                            (int)b.params.size(), b.width, b.height, b.T_ck.data(), Given(dst), dst.width, dst.height, alpha, grid_x, grid_y, &u_),
               "StereoUncertainty");
  }
  // the calibrator's cameras with the pair's rows and columns of the solution covariance at the current state
  StereoUncertainty(ViCalibrator& cal, int cam_a, int cam_b, const LinearCamera& dst, int grid_x, int grid_y, double alpha = 0.0) : gx_(grid_x), gy_(grid_y) {
    vc_checked(vc_stereo_uncertainty_create_for_cameras(cal.handle(), cam_a, cam_b, Given(dst), dst.width, dst.height, alpha, grid_x, grid_y, &u_), "StereoUncertainty");
  }
  ~StereoUncertainty() { vc_stereo_uncertainty_destroy(u_); }
  StereoUncertainty(const StereoUncertainty&) = delete;
  StereoUncertainty& operator=(const StereoUncertainty&) = delete;
  // host code, no device: W (7 x 12, row-major) = d(w_a, w_b, baseline) / d(w_ck_a, dp_a, w_ck_b, dp_b)
  static std::array<double, 84> PoseJacobian(const Se3& T_ck_a, const Se3& T_ck_b) {
    std::array<double, 84> W{};
    vc_checked(vc_stereo_pose_jacobian(T_ck_a.data(), T_ck_b.data(), W.data()), "PoseJacobian");
    return W;
  }
  // cov: n x n row-major in the layout q_a p_a K_a q_b p_b K_b, nullptr = the calibrator's; 1 to 8 depths
  void Run(const double* cov, double sigma_px, const std::vector<double>& depths) {
    n_depths_ = 0;
    vc_checked(vc_stereo_uncertainty_run(u_, cov, sigma_px, depths.data(), (int)depths.size()), "Run");
    n_depths_ = (int)depths.size();
  }
  // var: n_depths x gy x gx x 3 = (var_dv, var_d, var_Z), NaN at an invalid sample; flags: n_depths x gy x gx
  void Map(std::vector<double>* var, std::vector<unsigned char>* flags) {
    const size_t n = (size_t)gx_ * gy_ * (n_depths_ > 0 ? n_depths_ : 1);
    var->resize(3 * n); flags->resize(n);
    vc_checked(vc_stereo_uncertainty_get_map(u_, var->data(), flags->data()), "Map");
  }
  StereoUncertaintySummary Summary(int plane) {
    StereoUncertaintySummary s;
    vc_checked(vc_stereo_uncertainty_summary(u_, plane, &s.count, &s.invalid, &s.sum_var_dv, &s.sum_var_d, &s.sum_var_z, &s.max_var_dv, &s.worst), "Summary");
    return s;
  }
  // the variances of w_a (3), w_b (3) and of the baseline at the last run's covariance and sigma_px
  std::array<double, 7> PoseSigma() { std::array<double, 7> v{}; vc_checked(vc_stereo_uncertainty_get_pose_sigma(u_, v.data()), "PoseSigma"); return v; }
  double Baseline() { double b = 0.0; vc_checked(vc_stereo_uncertainty_get(u_, nullptr, nullptr, nullptr, &b, nullptr), "Baseline"); return b; }
  LinearCamera Destination(int dst_width, int dst_height) {
    LinearCamera d; d.width = dst_width; d.height = dst_height;
    vc_checked(vc_stereo_uncertainty_get(u_, nullptr, nullptr, d.fu_fv_u0_v0.data(), nullptr, nullptr), "Destination");
    return d;
  }
  std::array<double, 2> Time(int reps = 20) { std::array<double, 2> ms{{0, 0}}; vc_checked(vc_time_stereo_uncertainty(u_, reps, ms.data()), "Time"); return ms; }
  vc_stereo_uncertainty* handle() { return u_; }

 private:
  static const double* Given(const LinearCamera& d) { return (d.fu_fv_u0_v0[0] == 0.0 && d.fu_fv_u0_v0[1] == 0.0) ? nullptr : d.fu_fv_u0_v0.data(); }
  vc_stereo_uncertainty* u_ = nullptr;
  int gx_ = 0, gy_ = 0, n_depths_ = 0;
};

// Greedy D-optimal selection of the most informative views (vc_selector*): which candidate frames carry the information on the shared
// vision parameters, every frame's pose marginalised.  At most 64 shared columns.
struct Selection { std::vector<int> order; std::vector<double> gain, cum; double total = 0; };      // cum[k] / total: the share of the first k + 1 views
struct SelectionFrames { std::vector<int> status, corners, behind; };                                 // status: 0 usable, 1 underdetermined, 2 usable, corners behind
class Selector {
 public:
  // cams: model, params and pose are read; flags: per camera 1 rotation free | 2 translation free | 4 intrinsics free
  Selector(const std::vector<CameraAndPose>& cams, const std::vector<int>& flags, int device = 0) {
    const int n = (int)cams.size();
    std::vector<int> model(cams.size()), nparams(cams.size());
    std::vector<double> params(10 * cams.size(), 0.0), T_ck(7 * cams.size());
    for (size_t c = 0; c < cams.size(); ++c) {
      model[c] = cams[c].model; nparams[c] = (int)cams[c].params.size();
      for (size_t k = 0; k < cams[c].params.size() && k < 10; ++k) params[10 * c + k] = cams[c].params[k];
      for (int k = 0; k < 7; ++k) T_ck[7 * c + k] = cams[c].T_ck.data()[k];
    }
    vc_checked(flags.size() == cams.size() ? vc_selector_create(device, n, model.data(), params.data(), nparams.data(), T_ck.data(), flags.data(), &s_) : VC_ERR_BAD_ARG, "Selector");
  }
  // the calibrator's cameras, flags, frame poses and observation tiles at its host state
  explicit Selector(ViCalibrator& cal) {
    vc_checked(vc_selector_create_for_calibrator(cal.handle(), &s_), "Selector");
    n_frames_ = (int)cal.NumFrames();
  }
  ~Selector() { vc_selector_destroy(s_); }
  Selector(const Selector&) = delete;
  Selector& operator=(const Selector&) = delete;
  void AddTiles(int n_tiles, const int* tile_frame, const int* tile_cam, const long long* tile_off, const double* points, int n_points, const int* point_id) {
    vc_checked(vc_select_add_tiles(s_, n_tiles, tile_frame, tile_cam, tile_off, points, n_points, point_id), "AddTiles");
  }
  void SetPoses(const double* T_wk /* n_frames x 7 */, int n_frames) { vc_checked(vc_select_set_poses(s_, T_wk, n_frames), "SetPoses"); n_frames_ = n_frames; }
  Selection Run(int k, const std::vector<int>& start = {}, double prior = 1e-6) {
    vc_checked(vc_select_run(s_, k, start.empty() ? nullptr : start.data(), (int)start.size(), prior), "Run");
    Selection r;
    const size_t n = (size_t)(n_frames_ > 0 ? n_frames_ : 1);
    r.order.resize(n); r.gain.resize(n); r.cum.resize(n);
    int picked = 0;
    vc_checked(vc_select_get(s_, &picked, r.order.data(), r.gain.data(), r.cum.data(), &r.total), "Run");
    r.order.resize((size_t)picked); r.gain.resize((size_t)picked); r.cum.resize((size_t)picked);
    return r;
  }
  SelectionFrames Frames() {
    SelectionFrames f;
    const size_t n = (size_t)(n_frames_ > 0 ? n_frames_ : 1);
    f.status.resize(n); f.corners.resize(n); f.behind.resize(n);
    vc_checked(vc_select_frames(s_, f.status.data(), f.corners.data(), f.behind.data()), "Frames");
    return f;
  }
  // I: D x D row-major, unscaled; scale: D
  void FrameInformation(int frame, std::vector<double>* I, std::vector<double>* scale) {
    const size_t D = (size_t)Dim();
    I->resize(D * D); scale->resize(D);
    vc_checked(vc_select_frame_information(s_, frame, I->data(), scale->data()), "FrameInformation");
  }
  // the gains of all candidates in the last round that ran; -1 for frames selected before it, in the start set, or unusable
  std::vector<double> LastGains() {
    std::vector<double> g((size_t)(n_frames_ > 0 ? n_frames_ : 1));
    vc_checked(vc_select_last_gains(s_, g.data()), "LastGains");
    return g;
  }
  int Dim() { return vc_checked(vc_select_dim(s_), "Dim"); }
  int NumFrames() const { return n_frames_; }
  std::array<double, 3> Time(int reps = 20) { std::array<double, 3> ms{{0, 0, 0}}; vc_checked(vc_time_select(s_, reps, ms.data()), "Time"); return ms; }
  vc_selector* handle() { return s_; }

 private:
  vc_selector* s_ = nullptr;
  int n_frames_ = 0;
};

// A depth image of one camera of the rig registered into another (vc_regist*): the depth camera `src` into `dst`'s pixels by a forward warp
// with a depth test, and dst's 8-bit image into src's pixels with an occlusion test.  kind: 0 Z, 1 range; splat: 0 nearest, 1 footprint.
struct RegisterInfo { double R[9], t[3]; int src_size[2], dst_size[2]; double unit_src = 0, unit_dst = 0; int kind = 0, splat = 0; };
class Registrar {
 public:
  Registrar(const CameraAndPose& src, const CameraAndPose& dst, double unit_src = 0.001, double unit_dst = 0.001, int kind = 0, int splat = 0, int device = 0) {
    vc_checked(vc_registrar_create(device, src.model, src.params.data(), (int)src.params.size(), src.width, src.height, src.T_ck.data(), dst.model, dst.params.data(),
                                   (int)dst.params.size(), dst.width, dst.height, dst.T_ck.data(), unit_src, unit_dst, kind, splat, &r_), "Registrar");
  }
  Registrar(ViCalibrator& cal, int cam_s, int cam_d, double unit_src = 0.001, double unit_dst = 0.001, int kind = 0, int splat = 0) {
    vc_checked(vc_registrar_create_for_cameras(cal.handle(), cam_s, cam_d, unit_src, unit_dst, kind, splat, &r_), "Registrar");
  }
  ~Registrar() { vc_registrar_destroy(r_); }
  Registrar(const Registrar&) = delete;
  Registrar& operator=(const Registrar&) = delete;
  RegisterInfo Get() {
    RegisterInfo g; double units[2] = {0, 0};
    vc_checked(vc_register_get(r_, g.R, g.t, g.src_size, g.dst_size, units, &g.kind, &g.splat), "Get");
    g.unit_src = units[0]; g.unit_dst = units[1];
    return g;
  }
  // index (n x h_d x w_d) and counters (n x 8) may be nullptr; pitches and strides in bytes
  void Depth(int n, const unsigned short* src, int src_pitch, long long src_stride, unsigned short* dst, int dst_pitch, long long dst_stride, int* index = nullptr,
             long long* counters = nullptr) {
    vc_checked(vc_register_depth(r_, n, src, src_pitch, src_stride, dst, dst_pitch, dst_stride, index, counters), "Depth");
  }
  void DepthDevice(int n, const unsigned short* d_src, int src_pitch, long long src_stride, unsigned short* d_dst, int dst_pitch, long long dst_stride,
                   int* d_index = nullptr, long long* d_counters = nullptr) {
    vc_checked(vc_register_depth_device(r_, n, d_src, src_pitch, src_stride, d_dst, dst_pitch, dst_stride, d_index, d_counters), "DepthDevice");
  }
  void* Stream() { return vc_register_stream(r_); }      // hipStream_t
  void Color(int n, const unsigned short* depth, int depth_pitch, long long depth_stride, const unsigned char* color, int color_pitch, long long color_stride,
             double occl_tol, int fill, unsigned char* out, int out_pitch, long long out_stride, unsigned char* mask = nullptr) {
    vc_checked(vc_register_color(r_, n, depth, depth_pitch, depth_stride, color, color_pitch, color_stride, occl_tol, fill, out, out_pitch, out_stride, mask), "Color");
  }
  // rows (u, v, value) -> rows (q_x, q_y, m_d / unit_dst)
  void Points(int n, const double* in, double* out, unsigned char* valid = nullptr) { vc_checked(vc_register_points(r_, n, in, out, valid), "Points"); }
  std::array<double, 4> Time(int n_images = 8, int reps = 20) { std::array<double, 4> ms{{0, 0, 0, 0}}; vc_checked(vc_time_register(r_, n_images, reps, ms.data()), "Time"); return ms; }
  vc_registrar* handle() { return r_; }

 private:
  vc_registrar* r_ = nullptr;
};

// The range error of a depth camera measured against the calibration target and its correction (vc_depthcal*): frames with their poses are
// added to binned sums, a polynomial in the value plus an affine term per image cell is fitted from the sums, and depth images are corrected.
struct DepthCalOptions {
  double unit = 0.001; int kind = 0; double rect[4] = {0, 0, 1, 1}; int bins_x = 4, bins_y = 3; double v_ref = 1000.0, min_cos = 0.5, max_dev = 100.0;
};
struct DepthCalFit { int degree = 0; double c[3] = {0, 0, 0}, rms[3] = {0, 0, 0}; std::vector<double> a, b; std::vector<int> status; };
struct DepthCalSums { std::vector<double> sums; double totals[9]; long long counters[8]; long long n_frames = 0; };
class DepthCalibrator {
 public:
  DepthCalibrator(const CameraAndPose& cam, const DepthCalOptions& o, int device = 0) : cells_(o.bins_x * o.bins_y) {
    vc_checked(vc_depthcal_create(device, cam.model, cam.params.data(), (int)cam.params.size(), cam.width, cam.height, cam.T_ck.data(), o.unit, o.kind, o.rect, o.bins_x,
                                  o.bins_y, o.v_ref, o.min_cos, o.max_dev, &d_), "DepthCalibrator");
  }
  DepthCalibrator(ViCalibrator& cal, int cam, const DepthCalOptions& o) : cells_(o.bins_x * o.bins_y) {
    vc_checked(vc_depthcal_create_for_camera(cal.handle(), cam, o.unit, o.kind, o.rect, o.bins_x, o.bins_y, o.v_ref, o.min_cos, o.max_dev, &d_), "DepthCalibrator");
  }
  ~DepthCalibrator() { vc_depthcal_destroy(d_); }
  DepthCalibrator(const DepthCalibrator&) = delete;
  DepthCalibrator& operator=(const DepthCalibrator&) = delete;
  void Clear() { vc_checked(vc_depthcal_clear(d_), "Clear"); }
  // T_wk: n x 7; counters (n x 8) may be nullptr; pitch and stride in bytes
  void Add(int n, const unsigned short* depth, int pitch, long long stride, const double* T_wk, long long* counters = nullptr) {
    vc_checked(vc_depthcal_add(d_, n, depth, pitch, stride, T_wk, counters), "Add");
  }
  // y: n x h x w, rule: n x h x w; depth may be nullptr
  void Expected(int n, const double* T_wk, const unsigned short* depth, int pitch, long long stride, double* y, unsigned char* rule) {
    vc_checked(vc_depthcal_expected(d_, n, T_wk, depth, pitch, stride, y, rule), "Expected");
  }
  DepthCalSums Sums() {
    DepthCalSums s; s.sums.resize((size_t)cells_ * 9);
    vc_checked(vc_depthcal_sums(d_, s.sums.data(), s.totals, s.counters, &s.n_frames), "Sums");
    return s;
  }
  DepthCalFit Fit(int degree = 2, int min_count = 50, double min_spread = 0.02) { vc_checked(vc_depthcal_fit(d_, degree, min_count, min_spread), "Fit"); return GetFit(); }
  DepthCalFit GetFit() {
    DepthCalFit f; f.a.resize(cells_); f.b.resize(cells_); f.status.resize(cells_);
    vc_checked(vc_depthcal_get_fit(d_, f.c, f.a.data(), f.b.data(), f.status.data(), f.rms, &f.degree), "GetFit");
    return f;
  }
  void SetFit(int degree, const double c[3], const double* a, const double* b) { vc_checked(vc_depthcal_set_fit(d_, degree, c, a, b), "SetFit"); }
  // counters (n x 3: zeros in, corrected, out of range) may be nullptr; dst == src is allowed
  void Apply(int n, const unsigned short* src, int src_pitch, long long src_stride, unsigned short* dst, int dst_pitch, long long dst_stride, int interp = 0,
             long long* counters = nullptr) {
    vc_checked(vc_depthcal_apply(d_, n, src, src_pitch, src_stride, dst, dst_pitch, dst_stride, interp, counters), "Apply");
  }
  std::array<double, 3> Time(int n_images = 8, int reps = 20) { std::array<double, 3> ms{{0, 0, 0}}; vc_checked(vc_time_depthcal(d_, n_images, reps, ms.data()), "Time"); return ms; }
  int Cells() const { return cells_; }
  vc_depthcal* handle() { return d_; }

 private:
  vc_depthcal* d_ = nullptr;
  int cells_ = 0;
};

// The noise of an IMU from a log recorded at rest (vc_allan*): the overlapping Allan variance of six channels on the device, the averaging
// factors and the fit of white noise N, bias instability B and rate random walk K on the host.
struct AllanInfo { int n = 0, first = 0, count = 0; double tau0 = 0, dt_min = 0, dt_max = 0, means[6] = {0, 0, 0, 0, 0, 0}; long long irregular = 0; };
struct AllanFactors { std::vector<int> m; std::vector<double> rel_err; };
struct AllanCurve { std::vector<double> avar; std::vector<int> terms; };      // avar: 6 x n_m, channel-major (gx gy gz ax ay az)
struct AllanFitResult { double N = 0, B = 0, K = 0, rms_log = 0; int n_points = 0, mask = 0, status = 0; };
inline AllanFactors AllanFactorList(int n_used, int per_decade = 20, double max_fraction = 1.0 / 9.0) {
  int n_m = 0;
  vc_checked(vc_allan_factors(n_used, per_decade, max_fraction, 0, nullptr, nullptr, &n_m), "AllanFactorList");
  AllanFactors f; f.m.resize(n_m); f.rel_err.resize(n_m);
  vc_checked(vc_allan_factors(n_used, per_decade, max_fraction, n_m, f.m.data(), f.rel_err.data(), &n_m), "AllanFactorList");
  return f;
}
inline AllanFitResult AllanFit(const std::vector<double>& tau, const double* avar, const std::vector<double>& rel_err) {
  if (tau.empty() || tau.size() != rel_err.size()) throw std::runtime_error("vicalib_amd: AllanFit: array sizes disagree");
  double out[5]; AllanFitResult r;
  r.status = vc_checked(vc_allan_fit((int)tau.size(), tau.data(), avar, rel_err.data(), out, &r.mask), "AllanFit");
  r.N = out[0]; r.B = out[1]; r.K = out[2]; r.rms_log = out[3]; r.n_points = (int)out[4];
  return r;
}
class AllanAnalyzer {
 public:
  // gyro, accel: n x 3; time: n, strictly increasing
  AllanAnalyzer(int n, const double* gyro, const double* accel, const double* time, int device = 0) {
    vc_checked(vc_allan_create(device, n, gyro, accel, time, &a_), "AllanAnalyzer");
  }
  ~AllanAnalyzer() { vc_allan_destroy(a_); }
  AllanAnalyzer(const AllanAnalyzer&) = delete;
  AllanAnalyzer& operator=(const AllanAnalyzer&) = delete;
  AllanInfo Get() {
    AllanInfo i; int range[2] = {0, 0};
    vc_checked(vc_allan_get(a_, &i.n, &i.tau0, &i.dt_min, &i.dt_max, i.means, &i.irregular, range), "Get");
    i.first = range[0]; i.count = range[1];
    return i;
  }
  void SetRange(int first, int count) { vc_checked(vc_allan_set_range(a_, first, count), "SetRange"); }
  // the longest quiet stretch becomes the range; false (the range stays) when no window start is quiet
  bool Static(int window, double gyro_thr, double accel_thr, int* n_quiet = nullptr) {
    return vc_checked(vc_allan_static(a_, window, gyro_thr, accel_thr, nullptr, n_quiet), "Static") == 0;
  }
  AllanCurve Run(const std::vector<int>& m) {
    AllanCurve c; c.avar.resize(6 * m.size()); c.terms.resize(m.size());
    vc_checked(vc_allan_run(a_, (int)m.size(), m.data(), c.avar.data(), c.terms.data()), "Run");
    return c;
  }
  std::array<double, 2> Time(const std::vector<int>& m, int reps = 10) {
    std::array<double, 2> ms{{0, 0}};
    vc_checked(vc_time_allan(a_, (int)m.size(), m.data(), reps, ms.data()), "Time");
    return ms;
  }
  vc_allan* handle() { return a_; }

 private:
  vc_allan* a_ = nullptr;
};

}  // namespace visual_inertial_calibration
