// vicalib -- command-line calibration tool on libvicalib_amd.so, keeping the reference tool's command line
// (flags of src/vicalib-engine.cc:30-104 and src/vicalib-task.cc:19-51) and its outputs (cameras.xml, poses.csv,
// poses.txt).  What the reference does with HAL + Calibu image processing (grab images, find conics, match the
// grid) is outside the solver path; here the sensors are files:
//
//   -cam  detections://cam0.csv[,cam1.csv,...]   one file per camera channel, lines  frame,dot_id,u,v,X,Y,Z[,time]
//                                                (the format the reference prints with -output_conics,
//                                                 vicalib-task.cc:313-317; `time` is an optional 8th column)
//   -cam  file://dir/cam0_*.pgm[,dir/cam1_*.pgm]  (round 4) one glob of 8-bit PGM images per camera channel, sorted by name, one frame per
//                                                image -- HAL's FileReader URI of the reference's own usage line (main.cc:11).  Every
//                                                image goes through the GPU dot detector (vc_detector_find_conics) and the grid
//                                                association (vc_target_find): what VicalibTask::AddImageMeasurements does with
//                                                calibu::ImageProcessing / ConicFinder / TargetGridDot (vicalib-task.cc:263-330).
//                                                The target's large / small pattern comes from -grid_pattern_file (rows of 0 / 1), or
//                                                from -grid_height / -grid_width / -grid_seed through the library's own generator;
//                                                Calibu's presets and MakePattern are not in the reference tree.
//   -imu  csv://dir                              HAL CsvDriver layout: dir/accel.txt, dir/gyro.txt, dir/timestamp.txt
//
// Everything from "AddFrame" on is the reference's flow: start intrinsics per -models (vicalib-engine.cc:203-257) or
// -model_files, PnP seed pose per frame (vicalib-task.cc:335-348), Start(has_initial_guess) (vicalib-task.cc:226-234),
// 30 ms polling loop (vicalib-engine.cc:376-431), WriteCalibration (:353-372), success test (vicalib-task.cc:831-856).
//
// This file holds that flow: main() at the bottom lists the stages, each a function above it over the one `Run` they share.  The rest of the
// translation unit is in three headers beside it: vicalib_flags.hpp (flag definitions and parsing), vicalib_io.hpp (file readers and writers),
// vicalib_tools.hpp (the file-to-file tools and the outputs written behind a calibration).
#include <vicalib_amd.hpp>
#include "../vicalib_amd/csrc/vc_holdout_select.hpp"      // which frames -holdout_every keeps out (host arithmetic, no device code)
#include "../vicalib_amd/csrc/vc_allan.hpp"               // the noise model of -allan_imu evaluated at an averaging time (host arithmetic, no device code)

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <glob.h>
#include <sys/stat.h>
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

namespace vic = visual_inertial_calibration;

#include "vicalib_flags.hpp"
#include "vicalib_io.hpp"
#include "vicalib_tools.hpp"


// rotation matrix (row-major) -> unit quaternion [x y z w], w >= 0
static void RotationToQuat(const double* R, double* q) {
  const double tr = R[0] + R[4] + R[8];
  if (tr > 0.0) { const double s = 2.0 * std::sqrt(tr + 1.0); q[0] = (R[7] - R[5]) / s; q[1] = (R[2] - R[6]) / s; q[2] = (R[3] - R[1]) / s; q[3] = 0.25 * s; }
  else if (R[0] > R[4] && R[0] > R[8]) { const double s = 2.0 * std::sqrt(1.0 + R[0] - R[4] - R[8]); q[0] = 0.25 * s; q[1] = (R[1] + R[3]) / s; q[2] = (R[2] + R[6]) / s; q[3] = (R[7] - R[5]) / s; }
  else if (R[4] > R[8]) { const double s = 2.0 * std::sqrt(1.0 + R[4] - R[0] - R[8]); q[0] = (R[1] + R[3]) / s; q[1] = 0.25 * s; q[2] = (R[5] + R[7]) / s; q[3] = (R[2] - R[6]) / s; }
  else { const double s = 2.0 * std::sqrt(1.0 + R[8] - R[0] - R[4]); q[0] = (R[2] + R[6]) / s; q[1] = (R[5] + R[7]) / s; q[2] = 0.25 * s; q[3] = (R[3] - R[1]) / s; }
  const double n = (q[3] < 0.0 ? -1.0 : 1.0) / std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int k = 0; k < 4; ++k) q[k] *= n;
}
static void QuatMul(const double* a, const double* b, double* o) {
  const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  const double z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  o[0] = x; o[1] = y; o[2] = z; o[3] = w;
}
static void QuatRotate(const double* q, const double* v, double* o) {
  const double p[4] = {v[0], v[1], v[2], 0.0}, c[4] = {-q[0], -q[1], -q[2], q[3]};
  double t[4], r[4];
  QuatMul(q, p, t); QuatMul(t, c, r);
  o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
}
// poses [qx qy qz qw tx ty tz]: a b, and the inverse
static vic::Se3 Se3Mul(const vic::Se3& a, const vic::Se3& b) {
  vic::Se3 o;
  QuatMul(a.v.data(), b.v.data(), o.v.data());
  double t[3];
  QuatRotate(a.v.data(), b.v.data() + 4, t);
  for (int k = 0; k < 3; ++k) o.v[4 + k] = t[k] + a.v[4 + k];
  return o;
}
static vic::Se3 Se3Inverse(const vic::Se3& a) {
  vic::Se3 o;
  for (int k = 0; k < 3; ++k) o.v[k] = -a.v[k];
  o.v[3] = a.v[3];
  double t[3];
  QuatRotate(o.v.data(), a.v.data() + 4, t);
  for (int k = 0; k < 3; ++k) o.v[4 + k] = -t[k];
  return o;
}
static void RotationMatrix(const double* q, double* R) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}

// IMUCalibrationDiffer (vicalib-task.cc:807-829).  The reference compares with '<': it reports a difference when a bias moved by
// LESS than the limit in any component -- with start biases of zero (vicalib-task.cc:129) that is nearly every calibration, so
// -has_initial_guess makes its IsSuccessful() fail unless all six biases exceed the limits.  The exit status is part of the tool's
// behaviour: 'reference' reproduces it (and says so), 'corrected' compares the way the message reads.
static bool IMUCalibrationDiffer(const double* last, const double* current, bool reference_sense) {
  double diff[6];
  for (int i = 0; i < 6; ++i) diff[i] = last[i] - current[i];
  const double lg = FlagDouble("max_imu_gyro_diff"), la = FlagDouble("max_imu_accel_diff");
  auto out = [&](double d, double lim) { return reference_sense ? std::fabs(d) < lim : std::fabs(d) > lim; };
  for (int s = 0; s < 2; ++s) {                  // the gyroscope's three, then the accelerometer's
    const double* d = diff + 3 * s, lim = s ? la : lg;
    if (!out(d[0], lim) && !out(d[1], lim) && !out(d[2], lim)) continue;
    std::fprintf(stderr, "E IMU bias(es) for %s differ (%g, %g, %g ) more than expected (%g)%s\n", s ? "accelrometer" : "gyroscope", d[0], d[1], d[2], lim,
                 reference_sense ? " [reference comparison sense: '<', see -imu_diff_sense]" : "");
    return true;
  }
  return false;
}

// CameraCalibrationsDiffer (vicalib-task.cc:722-806)
static bool CameraCalibrationsDiffer(const vic::CameraAndPose& last, const vic::CameraAndPose& cur) {
  const char* names[4] = {"fx", "fy", "cx", "cy"};
  const char* lim[4] = {"max_fx_diff", "max_fy_diff", "max_cx_diff", "max_cy_diff"};
  for (int i = 0; i < 4; ++i)
    if (std::fabs(last.params[i] - cur.params[i]) > FlagDouble(lim[i])) { std::fprintf(stderr, "E %s differs too much (%g)\n", names[i], last.params[i] - cur.params[i]); return true; }
  if (cur.model == VC_MODEL_FOV && std::fabs(last.params[4] - cur.params[4]) > FlagDouble("max_fov_w_diff")) { std::fprintf(stderr, "E fov distortion differs too much\n"); return true; }
  if (cur.model == VC_MODEL_POLY3) {
    const char* l3[3] = {"max_poly3_diff_k1", "max_poly3_diff_k2", "max_poly3_diff_k3"};
    for (int i = 0; i < 3; ++i) if (std::fabs(last.params[4 + i] - cur.params[4 + i]) > FlagDouble(l3[i])) { std::fprintf(stderr, "E poly3 distortion differs too much\n"); return true; }
  }
  double d2 = 0;
  for (int i = 4; i < 7; ++i) d2 += (last.T_ck.v[i] - cur.T_ck.v[i]) * (last.T_ck.v[i] - cur.T_ck.v[i]);
  if (std::sqrt(d2) > FlagDouble("max_camera_trans_diff")) { std::fprintf(stderr, "E position of camera differs by %g\n", std::sqrt(d2)); return true; }
  double Ra[9], Rb[9], M[9];
  RotationMatrix(last.T_ck.data(), Ra); RotationMatrix(cur.T_ck.data(), Rb);
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { M[3 * i + j] = 0; for (int k = 0; k < 3; ++k) M[3 * i + j] += Ra[3 * k + i] * Rb[3 * k + j]; }
  const double ax = std::atan2(M[7], M[8]), ay = std::atan2(-M[6], std::sqrt(M[7] * M[7] + M[8] * M[8])), az = std::atan2(M[3], M[0]);
  const double lim_a = FlagDouble("max_camera_angle_diff");
  if (std::fabs(ax) > lim_a || std::fabs(ay) > lim_a || std::fabs(az) > lim_a) { std::fprintf(stderr, "E camera orientations are farther apart than expected\n"); return true; }
  return false;
}

// _T2Cart (vicalib-engine.cc:318-351): x y z roll pitch yaw
static void T2Cart(const double* T, double* c) {
  double R[9]; RotationMatrix(T, R);
  c[0] = T[4]; c[1] = T[5]; c[2] = T[6];
  c[3] = std::atan2(R[7], R[8]);
  const double det = -R[6] * R[6] + 1.0;
  c[4] = det <= 0 ? (R[6] > 0 ? -M_PI / 2 : M_PI / 2) : -std::asin(R[6]);
  c[5] = std::atan2(R[3], R[0]);
}

// -report_bins WxH, each 1..32
static bool ParseBins(const std::string& s, int* bx, int* by) {
  int a = 0, b = 0; char tail = 0;
  if (std::sscanf(s.c_str(), "%dx%d%c", &a, &b, &tail) != 2 || a < 1 || a > 32 || b < 1 || b > 32) return false;
  *bx = a; *by = b;
  return true;
}

// -holdout_every N: 0 or N >= 2
static bool ParseHoldoutEvery(const std::string& s, int* every) {
  int a = 0; char tail = 0;
  if (std::sscanf(s.c_str(), "%d%c", &a, &tail) != 1 || a < 0 || a == 1) return false;
  *every = a;
  return true;
}
static const char* HoldoutStatusName(int s) {
  static const char* names[] = {"converged", "max_iters", "underdetermined", "no_seed", "failed"};
  return s >= 0 && s < 5 ? names[s] : "?";
}

// ------------------------------------------------------------------------------------------- the run and what its stages share
// What the stages hand on.  Never copied: rank_corners and the held-out scoring keep Detection* into channels[c].det, which must not move once filled.
struct Run {
  int report_bx = 16, report_by = 12, holdout_every = 0;
  bool want_report = false, converting = false;
  UncertaintyOptions uncertainty; StereoUncertaintyOptions stereo_uncertainty; SelectOptions select; CompareOptions compare; ConvertOptions convert;
  RegisterOptions reg; DepthCalCli depthcal; AllanCli allan;
  std::vector<vic::CameraAndPose> compare_b;                                    // the rig of -compare_to (B)
  std::vector<std::string> cam_files; std::vector<Channel> channels; bool from_images = false;
  int grid_w = 0, grid_h = 0, img_w = 0, img_h = 0, rectify_a = 0, rectify_b = 1;
  ImuData imu; bool have_imu = false, calibrate_imu = false;
  std::vector<vic::CameraAndPose> input_cameras;
  std::vector<long> frame_ids, held_ids;
  double image_time_offset = 0.0, secs = 0.0;
  vic::SeedImuResult imu_seed;
  std::vector<std::unique_ptr<vic::ViCalibrator>> cals;                         // one per GPU; the shared parameters and statistics are identical on every rank
  std::vector<std::vector<const Detection*>> rank_corners;                      // (report) the detection behind every corner, in the order it was added
  std::vector<vic::VicalibFrame> all_frames;                                    // frames of all shards, in order
  std::vector<double> rmse;
  SelectHeld select_held;
  std::vector<std::string> incomplete;                                          // "-flag: the files are" of every output behind the result that failed
  // -dot_bias_rounds: the radius of every dot of the target by dot id, the detections as they were read (per channel, u v per detection), and
  // the last round's table for dot_bias.csv
  int dot_bias_rounds = 0;
  std::vector<double> dot_radius;
  std::vector<std::vector<double>> original_uv;
  struct DotBiasRow { long frame; int cam, dot; double bu, bv, radius_px; int status; };
  std::vector<DotBiasRow> dot_bias_rows;
  // -refine_target_rounds / -target_points: the target by dot id (x 3), as the detections name it (nominal) and as it is used (points); the last
  // round's corner counts and statuses for -refine_target_output
  int refine_rounds = 0;
  bool quiet_load = false;
  std::vector<double> target_nominal, target_points;
  std::vector<int> target_seen, target_corners, target_status;
};
// what a calibrator is rebuilt from between the rounds of -dot_bias_rounds: the result of the round before
struct Restart {
  std::vector<vic::CameraAndPose> cameras;
  std::vector<vic::VicalibFrame> frames;
  std::array<double, 6> biases, scale_factor;
  std::array<double, 2> gravity;
  double time_offset = 0.0;
};

// A stage that can end the program returns true to go on and false to end it with exit status *rc.  Stop says why on stderr.
__attribute__((format(printf, 3, 4))) static bool Stop(int* rc, int status, const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); std::vfprintf(stderr, fmt, ap); va_end(ap);
  *rc = status; return false;
}
static bool FlagError(int* rc, const std::string& what) { return Stop(rc, 1, "ERROR: %s\n", what.c_str()); }
// the end of a stand-alone mode: status 0, 1 (an error said in err) or 3 (no device)
static bool FinishMode(int* rc, int status, const char* what, const std::string& err) {
  if (status != 0) std::fprintf(stderr, "%s %s\n", status == 3 ? "F" : (std::string("E ") + what + " failed:").c_str(), err.c_str());
  *rc = status; return false;
}
// the cameras at the result, with the input's model and size
static std::vector<vic::CameraAndPose> CamerasAtResult(vic::ViCalibrator& cal, const std::vector<vic::CameraAndPose>& input_cameras) {
  std::vector<vic::CameraAndPose> a;
  for (size_t c = 0; c < input_cameras.size(); ++c) {
    a.push_back(cal.GetCamera(c));
    a[c].model = input_cameras[c].model; a[c].width = input_cameras[c].width; a[c].height = input_cameras[c].height;
  }
  return a;
}
// The covariance at the result, rank 0's (*dim x *dim; empty and 0 if it cannot be computed).  Collective when the frames are sharded: every rank
// linearises, on a thread of its own.
static std::vector<double> CovarianceOnEveryRank(const std::vector<std::unique_ptr<vic::ViCalibrator>>& cals, int* dim) {
  std::vector<std::vector<double>> covs(cals.size());
  std::vector<int> dims(cals.size(), 0);
  std::vector<std::thread> th;
  for (size_t r = 0; r < cals.size(); ++r) th.emplace_back([&, r] { covs[r] = cals[r]->GetSolutionCovariance(&dims[r]); });
  for (auto& t : th) t.join();
  *dim = dims[0];
  return covs[0];
}

// ------------------------------------------------------------------------------------------- the stages, in the order main() runs them
// Every flag that can be judged alone, before any file is opened, in a fixed order: the first thing wrong is the one reported.
static bool CheckFlags(Run& s, int* rc) {
  std::string err;
  if (!ParseBins(FlagString("report_bins"), &s.report_bx, &s.report_by))
    return FlagError(rc, "illegal value '" + FlagString("report_bins") + "' specified for flag 'report_bins': expected WIDTHxHEIGHT with both between 1 and 32");
  s.want_report = !FlagString("report_dir").empty() || FlagInt("report_worst") > 0;
  if (!ParseHoldoutEvery(FlagString("holdout_every"), &s.holdout_every))
    return FlagError(rc, "illegal value '" + FlagString("holdout_every") + "' specified for flag 'holdout_every': expected 0 (off) or N >= 2 (N = 1 would leave no frame to calibrate from)");
  if (FlagBool("seed_focal")) {
    if (!FlagString("model_files").empty()) return FlagError(rc, "-seed_focal and -model_files exclude each other: a model file brings its own focal length");
    if (!(FlagDouble("seed_focal_fit_px") >= 0.0)) return FlagError(rc, "illegal value for flag 'seed_focal_fit_px': expected at least 0");
  }
  s.dot_bias_rounds = (int)FlagInt("dot_bias_rounds");
  if (s.dot_bias_rounds < 0) return FlagError(rc, "illegal value for flag 'dot_bias_rounds': expected at least 0");
  if (s.dot_bias_rounds > 0) {
    if (FlagInt("gpus") > 1) return FlagError(rc, "-dot_bias_rounds needs -gpus 1: the rounds rebuild one calibrator from its own result");
    if (s.holdout_every > 0) return FlagError(rc, "-dot_bias_rounds and -holdout_every exclude each other: held-out frames would keep their bias");
    for (const char* f : {"dot_radius", "grid_large_rad", "grid_small_rad"})
      if (!(FlagDouble(f) >= 0.0) || !std::isfinite(FlagDouble(f)))
        return FlagError(rc, std::string("illegal value for flag '") + f + "' with -dot_bias_rounds: expected a radius in metres, at least 0");
  }
  s.refine_rounds = (int)FlagInt("refine_target_rounds");
  if (s.refine_rounds < 0) return FlagError(rc, "illegal value for flag 'refine_target_rounds': expected at least 0");
  if (s.refine_rounds > 0) {
    if (FlagInt("gpus") > 1) return FlagError(rc, "-refine_target_rounds needs -gpus 1: the rounds rebuild one calibrator from its own result");
    if (s.holdout_every > 0) return FlagError(rc, "-refine_target_rounds and -holdout_every exclude each other: held-out frames would be scored against another target");
    if (s.dot_bias_rounds > 0) return FlagError(rc, "-refine_target_rounds and -dot_bias_rounds exclude each other");
    if (!FlagString("imu").empty() && FlagBool("calibrate_imu"))
      return FlagError(rc, "-refine_target_rounds needs -nocalibrate_imu: the IMU ties the frame poses the target step marginalises freely");
    if (!(FlagDouble("refine_target_sigma") > 0.0) || !std::isfinite(FlagDouble("refine_target_sigma")) || !(1.0 / (FlagDouble("refine_target_sigma") * FlagDouble("refine_target_sigma")) < 1e300))
      return FlagError(rc, "illegal value for flag 'refine_target_sigma': expected a distance in metres, more than 0");
    if (FlagString("refine_target_output").empty()) return FlagError(rc, "-refine_target_rounds needs a file name in -refine_target_output");
  }
  if (FlagBool("seed_imu")) {
    if (FlagString("imu").empty()) return FlagError(rc, "-seed_imu needs -imu: there is no log to seed from");
    if (!FlagBool("calibrate_imu")) return FlagError(rc, "-seed_imu and -nocalibrate_imu exclude each other: nothing would use the seed");
    if (FlagBool("has_initial_guess")) return FlagError(rc, "-seed_imu and -has_initial_guess exclude each other: the guess is the start");
    if (!(FlagDouble("seed_imu_range") > 0.0) || !std::isfinite(FlagDouble("seed_imu_range"))) return FlagError(rc, "illegal value for flag 'seed_imu_range': expected more than 0");
    if (!std::isfinite(FlagDouble("seed_imu_step"))) return FlagError(rc, "illegal value for flag 'seed_imu_step': expected a number (0: the median sample interval)");
    if (!(FlagDouble("seed_imu_max_gap") > 0.0)) return FlagError(rc, "illegal value for flag 'seed_imu_max_gap': expected more than 0");
    if (FlagInt("seed_imu_min_intervals") < 1) return FlagError(rc, "illegal value for flag 'seed_imu_min_intervals': expected at least 1");
  }
  if (FlagString("seed_rig") != "off") {
    const std::string mode = FlagString("seed_rig");
    if (mode != "pnp" && mode != "mono") return FlagError(rc, "illegal value '" + mode + "' specified for flag 'seed_rig': expected off, pnp or mono");
    if (FlagBool("has_initial_guess")) return FlagError(rc, "-seed_rig and -has_initial_guess exclude each other: the guess is the start");
    if (!(FlagDouble("seed_rig_tol_deg") > 0.0) || !(FlagDouble("seed_rig_tol_deg") < 90.0)) return FlagError(rc, "illegal value for flag 'seed_rig_tol_deg': expected more than 0 and less than 90");
    if (FlagInt("seed_rig_min_support") < 1) return FlagError(rc, "illegal value for flag 'seed_rig_min_support': expected at least 1");
    if (!(FlagDouble("seed_rig_max_rmse") > 0.0)) return FlagError(rc, "illegal value for flag 'seed_rig_max_rmse': expected more than 0");
  }
  if (!UncertaintyFlags(&s.uncertainty, &err) || !StereoUncertaintyFlags(&s.stereo_uncertainty, &err) || !SelectFlags(&s.select, &err)) return FlagError(rc, err);
  // ---- -compare_models a.xml,b.xml: file against file, nothing is calibrated; -compare_to b.xml: read later, compared behind the results
  const bool comparing = !FlagString("compare_models").empty() || !FlagString("compare_to").empty();
  if (comparing) {
    if (!FlagString("compare_models").empty() && !FlagString("compare_to").empty()) return FlagError(rc, "-compare_models and -compare_to exclude each other");
    if (!CompareFlags(&s.compare, &err)) return FlagError(rc, err);
  }
  // ---- -convert_models in.xml -convert_to m[,m...]: file to file, nothing is calibrated; -convert_to alone: the result is converted behind it
  s.converting = !FlagString("convert_models").empty() || !FlagString("convert_to").empty();
  if (s.converting) {
    if (comparing) return FlagError(rc, "-convert_models / -convert_to and -compare_models / -compare_to exclude each other");
    if (!ConvertFlags(&s.convert, &err)) return FlagError(rc, err);
    if (!FlagString("compare_dir").empty()) {
      if (!CompareFlags(&s.compare, &err)) return FlagError(rc, err);
      s.compare.identity = true; s.compare.gx = s.convert.gx; s.compare.gy = s.convert.gy;      // (the conversion's own lattice; -compare_grid is not read)
    }
  }
  // ---- -register_models rig.xml -register_depth ...: file to file, nothing is calibrated; -register_depth alone: the result registers behind it
  if (!RegisterFlags(&s.reg, &err)) return FlagError(rc, err);
  if (s.reg.on && (!FlagString("compare_models").empty() || !FlagString("convert_models").empty()))
    return FlagError(rc, "-register_models / -register_depth and -compare_models / -convert_models exclude each other");
  // ---- -depthcal_models rig.xml -depthcal_poses ... / -depthcal_apply file: file to file, nothing is calibrated; -depthcal_depth alone: behind the result
  if (!DepthCalFlags(&s.depthcal, &err)) return FlagError(rc, err);
  if (s.depthcal.on && (!FlagString("compare_models").empty() || !FlagString("convert_models").empty() || !FlagString("register_models").empty()))
    return FlagError(rc, "-depthcal_models / -depthcal_depth / -depthcal_apply and -compare_models / -convert_models / -register_models exclude each other");
  // ---- -allan_imu csv://log -allan_dir dir: the IMU's noise from a static log, nothing is calibrated
  if (!AllanFlags(&s.allan, &err)) return FlagError(rc, err);
  return true;
}

// The modes that calibrate nothing: the first one asked for runs, and the program ends with its status (false).  true: none was asked for.
static bool RunStandAloneMode(Run& s, int* rc) {
  std::string err;
  std::vector<vic::CameraAndPose> a;
  auto read_rig = [&](const std::string& path, std::vector<vic::CameraAndPose>* cams) { return ReadRigFile(path, cams, &err) || Stop(rc, 1, "F %s\n", err.c_str()); };
  if (s.allan.on) return FinishMode(rc, AllanImu(s.allan, Device(), &err), "IMU noise characterisation", err);
  if (s.depthcal.apply) return FinishMode(rc, DepthCalApply(s.depthcal, Device(), &err), "depth correction", err);
  if (!s.depthcal.models.empty()) {
    std::vector<std::array<double, 7>> poses;
    if (!read_rig(s.depthcal.models, &a)) return false;
    if (!ReadPoseFile(s.depthcal.poses, &poses, &err)) return Stop(rc, 1, "F %s\n", err.c_str());
    return FinishMode(rc, DepthCalFit(a, poses, "-depthcal_poses", s.depthcal, Device(), &err), "depth calibration", err);
  }
  if (!FlagString("register_models").empty())
    return read_rig(FlagString("register_models"), &a) && FinishMode(rc, RegisterRig(a, s.reg, Device(), &err), "registration", err);
  if (!FlagString("convert_models").empty()) {
    if (!read_rig(FlagString("convert_models"), &a)) return false;
    if (!ConvertibleRig(a, s.convert, &err)) return FlagError(rc, err);
    return FinishMode(rc, ConvertRig(FlagString("convert_models"), a, s.convert, s.compare.identity ? &s.compare : nullptr, Device(), &err), "conversion", err);
  }
  if (!FlagString("compare_models").empty()) {
    const std::string& both = FlagString("compare_models");
    const size_t comma = both.find(',');
    if (comma == std::string::npos || comma == 0 || comma + 1 >= both.size() || both.find(',', comma + 1) != std::string::npos)
      return FlagError(rc, "illegal value '" + both + "' specified for flag 'compare_models': expected a.xml,b.xml");
    return read_rig(both.substr(0, comma), &a) && read_rig(both.substr(comma + 1), &s.compare_b) &&
           FinishMode(rc, CompareRigs(a, s.compare_b, s.compare, Device(), &err), "comparison", err);
  }
  return true;
}

// the target of image input (vicalib-engine.cc:453-465): its pattern from a file, or generated from -grid_height / -grid_width / -grid_seed
static bool ReadTarget(Run& s, const std::string& preset, TargetSpec* tg, int* rc) {
  tg->rows = s.grid_h; tg->cols = s.grid_w; tg->spacing = FlagDouble("grid_spacing");
  if (!FlagString("grid_pattern_file").empty()) {
    std::ifstream pf(FlagString("grid_pattern_file"));
    if (!pf) return Stop(rc, 1, "F cannot open grid pattern file %s\n", FlagString("grid_pattern_file").c_str());
    std::string line; std::vector<double> v; tg->rows = 0; tg->cols = 0;
    while (std::getline(pf, line)) {
      if (line.empty() || line[0] == '#') continue;
      if (!ParseNumbers(line, &v) || v.empty()) continue;
      if (tg->cols && (int)v.size() != tg->cols) return Stop(rc, 1, "F grid pattern file: rows of different length\n");
      tg->cols = (int)v.size(); ++tg->rows;
      for (double x : v) tg->pattern.push_back(x != 0.0 ? 1 : 0);
    }
    if (tg->rows < 2 || tg->cols < 2) return Stop(rc, 1, "F grid pattern file holds no pattern\n");
    s.grid_w = tg->cols; s.grid_h = tg->rows;
  } else if (!preset.empty()) {
    return Stop(rc, 1, "F -grid_preset %s with image input: the presets' large / small patterns live in Calibu, which is not part of the reference tree -- "
                       "pass the printed target's pattern with -grid_pattern_file (or generate a target with -grid_height / -grid_width / -grid_seed)\n", preset.c_str());
  } else {
    tg->pattern.resize((size_t)tg->rows * tg->cols);
    vc_target_make_pattern(tg->rows, tg->cols, (unsigned)FlagInt("grid_seed"), tg->pattern.data());
  }
  return true;
}

// The rig of -compare_to, the grid, the camera channels (detection files, or images through the dot detector on -device) and the IMU log.
static bool ReadSensors(Run& s, int* rc) {
  std::string err;
  if (!FlagString("compare_to").empty() && !ReadRigFile(FlagString("compare_to"), &s.compare_b, &err)) return Stop(rc, 1, "F %s\n", err.c_str());
  if (FlagString("cam").empty()) return Stop(rc, 1, "F No camera URI given\n");      // vicalib-engine.cc:445
  // ---- grid (vicalib-engine.cc:449-464): the detections already carry X,Y,Z; the preset only bounds the dot ids ----
  s.grid_w = (int)FlagInt("grid_width"); s.grid_h = (int)FlagInt("grid_height");
  const std::string preset = FlagString("grid_preset");
  if (!preset.empty()) {
    if (preset == "small" || preset == "0" || preset == "letter") { s.grid_w = 19; s.grid_h = 10; }
    else if (preset == "large" || preset == "1") { s.grid_w = 36; s.grid_h = 25; }
    else if (preset == "medium") { s.grid_w = 1 << 15; s.grid_h = 1; }     // size not recorded in the reference tree: no bound on dot ids
    else return Stop(rc, 1, "F Unknown grid preset %s\n", preset.c_str());
  }
  s.cam_files = Split(StripScheme(FlagString("cam")), ',');
  s.channels.resize(s.cam_files.size());
  s.from_images = FlagString("cam").compare(0, 7, "file://") == 0;      // HAL's FileReader scheme (main.cc:11)
  if (s.from_images) {
    TargetSpec tg;
    if (!ReadTarget(s, preset, &tg, rc)) return false;
    for (size_t c = 0; c < s.cam_files.size(); ++c) {
      int w = 0, h = 0;
      if (!ReadImages(s.cam_files[c], tg, Device(), &s.channels[c], &w, &h, &err)) return Stop(rc, err.find("HIP device") != std::string::npos ? 3 : 1, "F %s\n", err.c_str());
      s.img_w = std::max(s.img_w, w); s.img_h = std::max(s.img_h, h);
    }
  } else
  for (size_t c = 0; c < s.cam_files.size(); ++c)
    if (!ReadDetections(s.cam_files[c], &s.channels[c], &err)) return Stop(rc, 1, "F %s\n", err.c_str());
  const size_t n_cam = s.channels.size();
  if (!FlagString("rectify_dir").empty()) {
    if (n_cam < 2) return Stop(rc, 1, "E -rectify_dir needs two cameras (-cam has %zu)\n", n_cam);
    if (!ParseRectifyCams(FlagString("rectify_cams"), n_cam, &s.rectify_a, &s.rectify_b))
      return Stop(rc, 1, "E illegal value '%s' specified for flag 'rectify_cams': expected a,b, two different cameras below %zu\n", FlagString("rectify_cams").c_str(), n_cam);
    if (!(FlagDouble("rectify_alpha") >= 0.0 && FlagDouble("rectify_alpha") <= 1.0)) return Stop(rc, 1, "E illegal value for flag 'rectify_alpha': expected 0 ... 1\n");
  }
  s.have_imu = !FlagString("imu").empty();
  if (s.have_imu && !ReadImu(StripScheme(FlagString("imu")), FlagBool("use_system_time"), &s.imu, &err)) return Stop(rc, 1, "F %s\n", err.c_str());
  s.calibrate_imu = FlagBool("calibrate_imu");
  if (s.calibrate_imu && !s.have_imu) { std::fprintf(stderr, "W -calibrate_imu without -imu: calibrating the cameras only\n"); s.calibrate_imu = false; }
  return true;
}

// ---- -dot_bias_rounds: the radius of every dot of the target by dot id (row * grid_width + col).  -dot_radius gives all dots one radius; else
// a dot is large or small by the target's pattern: -grid_pattern_file, or generated from -grid_height / -grid_width (a preset's, with
// -grid_preset) and -grid_seed by the library's own generator, as for image input
static bool DotRadii(Run& s, int* rc) {
  if (FlagDouble("dot_radius") > 0.0) { s.dot_radius.assign((size_t)s.grid_w * s.grid_h, FlagDouble("dot_radius")); return true; }
  if (FlagString("grid_pattern_file").empty() && FlagString("grid_preset") == "medium")
    return Stop(rc, 1, "F -dot_bias_rounds with -grid_preset medium: the preset's size is not known here -- pass the target's pattern with -grid_pattern_file, or -dot_radius\n");
  TargetSpec tg;
  if (!ReadTarget(s, "", &tg, rc)) return false;
  for (int big : tg.pattern) s.dot_radius.push_back(FlagDouble(big ? "grid_large_rad" : "grid_small_rad"));
  return true;
}

// ---- start cameras (vicalib-engine.cc:162-257), and what the outputs behind the result can be told about them before any solve ------------------
static bool StartCameras(Run& s, int* rc) {
  std::string err;
  const size_t n_cam = s.channels.size();
  std::vector<std::string> models = Split(FlagString("models"), ','), model_files = Split(FlagString("model_files"), ',');
  if (model_files.empty() && models.size() < n_cam) {
    std::fprintf(stderr, "I Only %zu models declared; need one for all the %zu channels; assuming poly3\n", models.size(), n_cam);
    models.resize(n_cam, "poly3");
  }
  const int W = s.img_w > 0 ? s.img_w : (int)FlagInt("image_width"), H = s.img_h > 0 ? s.img_h : (int)FlagInt("image_height");      // (images carry their size)
  for (const std::string& mf : model_files) {
    vic::CameraAndPose cam;
    if (!ReadModelFile(mf, &cam, &err)) return Stop(rc, 1, "F %s\n", err.c_str());
    if (cam.width == 0) { cam.width = W; cam.height = H; }
    s.input_cameras.push_back(cam);
  }
  if (model_files.empty()) for (const std::string& type : models) {
    vic::CameraAndPose cam;
    cam.model = ModelId(type);
    if (cam.model < 0) return Stop(rc, 1, "F camera model '%s' is not supported by this build (fov, poly2, poly3, rational6, kb4, linear)\n", type.c_str());
    cam.width = W; cam.height = H;
    cam.params = {300, 300, W / 2.0, H / 2.0};
    if (cam.model == VC_MODEL_FOV) cam.params.push_back(0.2);
    else cam.params.resize(cam.model == VC_MODEL_POLY2 ? 6 : cam.model == VC_MODEL_POLY3 ? 7 : cam.model == VC_MODEL_KB4 ? 8 : cam.model == VC_MODEL_RATIONAL6 ? 10 : 4, 0.0);
    s.input_cameras.push_back(cam);
  }
  if (s.input_cameras.size() < n_cam) return Stop(rc, 1, "F %zu camera models for %zu channels\n", s.input_cameras.size(), n_cam);
  s.input_cameras.resize(n_cam);
  if (s.converting && !ConvertibleRig(s.input_cameras, s.convert, &err)) return FlagError(rc, err);
  if (!s.uncertainty.dir.empty()) {
    if (!FlagBool("calibrate_intrinsics")) return Stop(rc, 1, "F -uncertainty_dir needs -calibrate_intrinsics: fixed intrinsics have no covariance\n");
    for (size_t c = 0; c < n_cam; ++c)
      if (s.uncertainty.gx > s.input_cameras[c].width || s.uncertainty.gy > s.input_cameras[c].height) return Stop(rc, 1, "F camera %zu: -uncertainty_grid exceeds the image\n", c);
  }
  if (!s.stereo_uncertainty.dir.empty()) {
    const StereoUncertaintyOptions& su = s.stereo_uncertainty;
    if ((size_t)su.a >= n_cam || (size_t)su.b >= n_cam)
      return Stop(rc, 1, "E illegal value '%s' specified for flag 'stereo_uncertainty_cams': expected two cameras below %zu\n", FlagString("stereo_uncertainty_cams").c_str(), n_cam);
    if (!FlagBool("calibrate_intrinsics")) return Stop(rc, 1, "F -stereo_uncertainty_dir needs -calibrate_intrinsics: fixed intrinsics have no covariance\n");
    if (su.gx > s.input_cameras[su.a].width || su.gy > s.input_cameras[su.a].height) return Stop(rc, 1, "F -stereo_uncertainty_grid exceeds the image of camera %d\n", su.a);
  }
  if (!s.compare_b.empty() && !ComparableRigs(s.input_cameras, s.compare_b, s.compare, &err)) return Stop(rc, 1, "F -compare_to: %s\n", err.c_str());
  return true;
}

// ---- frames: union of the frame ids, -frame_skip, -num_vicalib_frames (vicalib-engine.cc:540-590); then -holdout_every N: every Nth surviving frame
// is not a frame of the problem (vc_holdout_select.hpp), it is scored afterwards.  The IMU stream is unchanged: the blocks simply span the gaps
static bool ChooseFrames(Run& s, int* rc) {
  std::set<long> ids;
  for (const Channel& ch : s.channels) for (const Detection& d : ch.det) ids.insert(d.frame);
  const long skip = FlagInt("frame_skip"), limit = FlagInt("num_vicalib_frames");
  long k = 0;
  for (long id : ids) {
    if (skip > 0 && (k++ % (skip + 1)) != 0) continue;
    if (limit >= 0 && (long)s.frame_ids.size() >= limit) break;
    s.frame_ids.push_back(id);
  }
  if (s.frame_ids.empty()) return Stop(rc, 1, "F no usable frames in the detections\n");
  if (s.holdout_every > 0) {
    if (!vc::holdout_every_ok((long long)s.frame_ids.size(), s.holdout_every))
      return FlagError(rc, "illegal value '" + std::to_string(s.holdout_every) + "' specified for flag 'holdout_every': it leaves fewer than 2 of the " +
                           std::to_string(s.frame_ids.size()) + " frames to calibrate from");
    std::vector<long> fit;
    for (size_t i = 0; i < s.frame_ids.size(); ++i) (vc::holdout_is_held((long long)i, s.holdout_every) ? s.held_ids : fit).push_back(s.frame_ids[i]);
    s.frame_ids.swap(fit);
  }
  return true;
}

// ---- -seed_focal: fx = fy of every camera from the homographies of its views in the frames that will be calibrated (held-out frames are
// not among them), one batch on -device; the one result serves every rank
static bool SeedFocal(Run& s, int* rc) {
  const size_t n_cam = s.channels.size();
  const std::map<long, int> fit_index = FrameIndex(s.frame_ids);
  std::vector<int> view_cam, view_off(1, 0);
  std::vector<double> pp, radius, pw, pc;
  const double frac = FlagDouble("seed_focal_radius");
  for (size_t c = 0; c < n_cam; ++c) {
    const double w = s.input_cameras[c].width, h = s.input_cameras[c].height;
    pp.insert(pp.end(), {w / 2.0, h / 2.0});
    radius.push_back(frac > 0.0 ? frac * 0.5 * std::sqrt(w * w + h * h) : 0.0);
    for (const auto& kv : DetectionsByFrame(s.channels[c], fit_index, s.grid_w * s.grid_h)) {
      AppendCorners(kv.second, &pw, &pc);
      view_cam.push_back((int)c); view_off.push_back((int)(pc.size() / 2));
    }
  }
  vic::SeedFocalResult sf;
  try { sf = vic::SeedFocalBatch(Device(), view_cam, pp, radius, view_off, pw, pc, 4, FlagDouble("seed_focal_fit_px")); }
  catch (const std::exception& e) { return Stop(rc, 3, "F -seed_focal: %s (device %d)\n", e.what(), Device()); }
  for (size_t c = 0; c < n_cam; ++c) {
    int total = 0;
    std::vector<double> fv;
    for (size_t v = 0; v < view_cam.size(); ++v) {
      if (view_cam[v] != (int)c) continue;
      ++total;
      if (sf.view_status[v] == 0 && std::isfinite(sf.view_f[v])) fv.push_back(sf.view_f[v]);
    }
    std::vector<double>& params = s.input_cameras[c].params;
    if (sf.cam_status[c] == 0) {
      params[0] = params[1] = sf.cam_f[c];
      std::sort(fv.begin(), fv.end());
      if (fv.empty()) std::fprintf(stderr, "I camera %zu: focal length seed %.2f px from %d of %d views\n", c, sf.cam_f[c], sf.cam_views[c], total);
      else std::fprintf(stderr, "I camera %zu: focal length seed %.2f px from %d of %d views (single views: %.2f .. %.2f px, median %.2f, %zu of them tilted enough)\n",
                        c, sf.cam_f[c], sf.cam_views[c], total, fv.front(), fv.back(), fv[fv.size() / 2], fv.size());
    } else {
      const char* why = sf.cam_status[c] == 1 ? "no usable view" : sf.cam_status[c] == 2 ? "the target was never tilted against the image plane" : "the views give no positive focal length";
      std::fprintf(stderr, "W camera %zu: no focal length seed (%s, %d of %d views usable); keeping fx = fy = %g\n", c, why, sf.cam_views[c], total, params[0]);
    }
  }
  return true;
}

// ---- -seed_rig pnp | mono: T_ck of every camera but the first from the views it shares with the others (vc_seed_rig: a vote among the per-frame
// relative poses), once on -device over the frames that will be calibrated, before any calibrator of the joint solve exists; the one result serves
// every rank.  pnp: the views are one PnP batch at the start intrinsics.  mono: every camera is calibrated alone first (identity pose, the frames
// where it has >= 4 corners, PnP seeds, vision only); a usable result gives the camera's start intrinsics and, as T_cw = T_wk^-1, its views.
static bool SeedRig(Run& s, int* rc) {
  const size_t n_cam = s.channels.size(), n_frames = s.frame_ids.size();
  if (n_cam < 2) { std::fprintf(stderr, "I -seed_rig: one camera, nothing to seed\n"); return true; }
  const bool mono = FlagString("seed_rig") == "mono";
  const std::map<long, int> fit_index = FrameIndex(s.frame_ids);
  std::vector<unsigned char> view_ok(n_frames * n_cam, 0);
  std::vector<double> view_T(7 * n_frames * n_cam, 0.0);
  auto set_view = [&](size_t k, size_t c, const double* T_cw) {
    for (int j = 0; j < 7; ++j) view_T[7 * (k * n_cam + c) + j] = T_cw[j];
    view_ok[k * n_cam + c] = 1;
  };
  if (!mono) {
    std::vector<int> view_model, view_off(1, 0), view_frame, view_cam;
    std::vector<double> view_K, pw, pc;
    for (size_t c = 0; c < n_cam; ++c) {
      const vic::CameraAndPose& cam = s.input_cameras[c];
      for (const auto& kv : DetectionsByFrame(s.channels[c], fit_index, s.grid_w * s.grid_h)) {
        if (kv.second.size() < 4) continue;
        AppendCorners(kv.second, &pw, &pc);
        view_model.push_back(cam.model); view_off.push_back((int)(pc.size() / 2)); view_frame.push_back(kv.first); view_cam.push_back((int)c);
        for (size_t j = 0; j < 10; ++j) view_K.push_back(j < cam.params.size() ? cam.params[j] : 0.0);
      }
    }
    const int nv = (int)view_frame.size();
    std::vector<double> T_cw(7 * (size_t)nv + 7, 0.0), rms((size_t)nv + 1, 0.0);
    std::vector<int> n_in((size_t)nv + 1, 0), pnp_status((size_t)nv + 1, -1);
    const int q = nv > 0 ? vc_pnp_planar_batch(Device(), nv, view_model.data(), view_K.data(), view_off.data(), pw.data(), pc.data(), (int)FlagInt("pnp_ransac_its"),
                                               FlagDouble("pnp_ransac_tol"), T_cw.data(), rms.data(), n_in.data(), nullptr, pnp_status.data())
                         : VC_OK;
    if (q == VC_ERR_NO_DEVICE) return Stop(rc, 3, "F -seed_rig: no HIP device %d\n", Device());
    if (q != VC_OK) { std::fprintf(stderr, "W -seed_rig: the pose batch failed (status %d); starting without the seed\n", q); return true; }
    for (int v = 0; v < nv; ++v)
      if (pnp_status[v] == 0) set_view((size_t)view_frame[v], (size_t)view_cam[v], &T_cw[7 * (size_t)v]);
  } else {
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t c = 0; c < n_cam; ++c) {
      std::unique_ptr<vic::ViCalibrator> cal;
      try { cal.reset(new vic::ViCalibrator(Device())); }
      catch (const std::exception& e) { return Stop(rc, 3, "F -seed_rig: %s (device %d)\n", e.what(), Device()); }
      const double zeros[6] = {0, 0, 0, 0, 0, 0}, ones[6] = {1, 1, 1, 1, 1, 1};
      cal->SetSigmas(FlagDouble("gyro_sigma"), FlagDouble("accel_sigma"));
      cal->SetBiases(zeros); cal->SetScaleFactor(ones);
      cal->FixCameraIntrinsics(!FlagBool("calibrate_intrinsics"));
      vic::CameraAndPose alone = s.input_cameras[c];
      alone.T_ck = vic::Se3();
      if (cal->AddCamera(alone) < 0) return Stop(rc, 1, "F AddCamera failed (model %s, %zu parameters)\n", ModelName(alone.model), alone.params.size());
      std::vector<int> frame_of;                                                             // the calibrator's frame -> the run's
      std::vector<double> pw, pc;
      vic::Se3 placeholder; placeholder.v = {{0, 0, 0, 1, 0, 0, 1000}};
      for (const auto& kv : DetectionsByFrame(s.channels[c], fit_index, s.grid_w * s.grid_h)) {
        if (kv.second.size() < 4) continue;
        const int f = cal->AddFrame(placeholder, FrameTime(s.channels, s.frame_ids[(size_t)kv.first]));
        pw.clear(); pc.clear();
        AppendCorners(kv.second, &pw, &pc);
        cal->AddObservations((size_t)f, 0, (int)kv.second.size(), pw.data(), pc.data());
        frame_of.push_back(kv.first);
      }
      bool usable = frame_of.size() >= 2;
      double rmse = 0.0; unsigned iters = 0;
      vic::CameraAndPose got;
      if (usable) {
        cal->SetPnPRansac((int)FlagInt("pnp_ransac_its"), FlagDouble("pnp_ransac_tol"));
        cal->SetPnPDevice(FlagBool("pnp_device"));
        cal->InitFramePosesPnP();
        cal->SetOptimizationFlags(false, false, true, false);
        cal->SetFunctionTolerance(FlagDouble("function_tolerance"));
        cal->SetMaxIters((int)FlagInt("max_iters"));
        cal->SetCalibrateImu(false);
        cal->SetRemoveOutliers(FlagBool("remove_outliers"), FlagDouble("outlier_threshold"));
        cal->Start();
        while (cal->IsRunning()) std::this_thread::sleep_for(std::chrono::milliseconds(2));
        cal->Stop();
        rmse = cal->GetCameraProjRMSE()[0]; iters = cal->GetNumIterations();
        got = cal->GetCamera(0);
        usable = std::isfinite(rmse) && rmse <= FlagDouble("seed_rig_max_rmse");
        for (double p : got.params) usable = usable && std::isfinite(p);
      }
      if (!usable) {
        std::fprintf(stderr, "W -seed_rig: camera %zu alone is not usable (%zu frames, RMSE %.4g px above %g or not finite); it keeps its start and has no views in the seed\n",
                     c, frame_of.size(), rmse, FlagDouble("seed_rig_max_rmse"));
        continue;
      }
      s.input_cameras[c].params = got.params;
      size_t n_views = 0;
      for (size_t f = 0; f < frame_of.size(); ++f) {
        const vic::Se3 T_cw = Se3Inverse(cal->GetFrame(f).t_wp_);
        bool finite = true;
        for (double p : T_cw.v) finite = finite && std::isfinite(p);
        if (finite) { set_view((size_t)frame_of[f], c, T_cw.data()); ++n_views; }
      }
      std::fprintf(stderr, "I -seed_rig: camera %zu alone: RMSE %.4f px after %u iterations, %zu views\n", c, rmse, iters, n_views);
    }
    std::fprintf(stderr, "I -seed_rig: %zu cameras calibrated alone in %.3f s\n", n_cam, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  }
  vic::SeedRigResult r;
  try { r = vic::SeedRig(Device(), (int)n_cam, view_ok, view_T, FlagDouble("seed_rig_tol_deg"), (int)FlagInt("seed_rig_min_support")); }
  catch (const std::exception& e) {
    if (std::string(e.what()).find("status -1)") != std::string::npos) return Stop(rc, 3, "F -seed_rig: no HIP device %d\n", Device());
    std::fprintf(stderr, "W -seed_rig: %s; starting without the seed\n", e.what());
    return true;
  }
  for (size_t c = 1; c < n_cam; ++c) {
    if (r.cam_status[c] != 0) {
      std::fprintf(stderr, "W -seed_rig: camera %zu is not connected to camera 0 by a pair with enough agreeing frames; it keeps its pose\n", c);
      continue;
    }
    vic::Se3 T_c0;
    for (int j = 0; j < 7; ++j) T_c0.v[j] = r.cam_T_c0[7 * c + j];
    s.input_cameras[c].T_ck = Se3Mul(T_c0, s.input_cameras[0].T_ck);
    const int par = r.cam_parent[c], a = std::min(par, (int)c), b = std::max(par, (int)c);
    const size_t p = (size_t)(a * ((int)n_cam - 1) - (a * (a - 1)) / 2 + (b - a - 1));
    const double* q = T_c0.v.data();
    std::fprintf(stderr, "I -seed_rig: camera %zu: parent %d, baseline %.4f m, angle %.3f degrees, support %d / %d shared frames, rms %.4f degrees %.5f m, "
                         "T_c0 [qx qy qz qw tx ty tz] %.9f %.9f %.9f %.9f %.6f %.6f %.6f\n", c, par,
                 std::sqrt(q[4] * q[4] + q[5] * q[5] + q[6] * q[6]), 2.0 * std::atan2(std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), std::fabs(q[3])) * 180.0 / M_PI,
                 r.pair_support[p], r.pair_shared[p], r.pair_rms_deg[p], r.pair_rms_m[p], q[0], q[1], q[2], q[3], q[4], q[5], q[6]);
  }
  return true;
}

// initial time offset (vicalib-task.cc:638-662): with system time the clocks are already aligned
static double InitialTimeOffset(const Run& s) {
  if (s.calibrate_imu && FlagBool("find_time_offset") && !FlagBool("use_system_time") && !s.imu.time.empty()) return s.imu.time[0] - FrameTime(s.channels, s.frame_ids[0]);
  return 0.0;
}

// ---- -seed_imu: R_ck of camera 0, the time offset, the gyro bias and gravity from the rates of camera 0's PnP rotations against the gyro's,
// one batch on -device before any calibrator exists; the one result serves every rank.  Any status but 0: a W line, today's start.
static bool SeedImu(Run& s, int* rc) {
  const vic::CameraAndPose& cam0 = s.input_cameras[0];
  const size_t n_frames = s.frame_ids.size();
  const std::map<int, std::vector<const Detection*>> per_frame = DetectionsByFrame(s.channels[0], FrameIndex(s.frame_ids), s.grid_w * s.grid_h);
  std::vector<int> view_model, view_off(1, 0), view_frame;
  std::vector<double> view_K, pw, pc, frame_t(n_frames), frame_q(4 * n_frames, 0.0);
  std::vector<unsigned char> frame_ok(n_frames, 0);
  for (size_t k = 0; k < n_frames; ++k) {
    frame_t[k] = FrameTime(s.channels, s.frame_ids[k]) + s.image_time_offset;      // the time the calibrators get
    frame_q[4 * k + 3] = 1.0;
    auto it = per_frame.find((int)k);
    if (it == per_frame.end() || it->second.size() < 4) continue;
    AppendCorners(it->second, &pw, &pc);
    view_model.push_back(cam0.model); view_off.push_back((int)(pc.size() / 2)); view_frame.push_back((int)k);
    for (size_t j = 0; j < 10; ++j) view_K.push_back(j < cam0.params.size() ? cam0.params[j] : 0.0);
  }
  const int nv = (int)view_frame.size();
  std::vector<double> T_cw(7 * (size_t)nv + 7, 0.0), rms((size_t)nv + 1, 0.0);
  std::vector<int> n_in((size_t)nv + 1, 0), pnp_status((size_t)nv + 1, -1);
  int q = nv > 0 ? vc_pnp_planar_batch(Device(), nv, view_model.data(), view_K.data(), view_off.data(), pw.data(), pc.data(), (int)FlagInt("pnp_ransac_its"),
                                       FlagDouble("pnp_ransac_tol"), T_cw.data(), rms.data(), n_in.data(), nullptr, pnp_status.data())
                 : VC_OK;
  if (q == VC_ERR_NO_DEVICE) return Stop(rc, 3, "F -seed_imu: no HIP device %d\n", Device());
  int n_ok = 0;
  for (int v = 0; v < nv && q == VC_OK; ++v) {
    if (pnp_status[v] != 0) continue;
    const size_t k = (size_t)view_frame[v];
    for (int j = 0; j < 3; ++j) frame_q[4 * k + j] = -T_cw[7 * (size_t)v + j];      // R_wc = R_cw^T
    frame_q[4 * k + 3] = T_cw[7 * (size_t)v + 3];
    frame_ok[k] = 1; ++n_ok;
  }
  vic::SeedImuResult& seed = s.imu_seed;
  if (q == VC_OK) {
    try {
      seed = vic::SeedImu(Device(), frame_t, frame_q, frame_ok, s.imu.time, s.imu.gyro, s.imu.accel, FlagDouble("seed_imu_range"), FlagDouble("seed_imu_step"), 8,
                          FlagDouble("seed_imu_max_gap"), (int)FlagInt("seed_imu_min_intervals"));
    } catch (const std::exception& e) {
      if (std::string(e.what()).find("status -1)") != std::string::npos) return Stop(rc, 3, "F -seed_imu: no HIP device %d\n", Device());
      std::fprintf(stderr, "W -seed_imu: %s; starting without the seed\n", e.what());
    }
  } else std::fprintf(stderr, "W -seed_imu: the pose batch of camera 0 failed (status %d); starting without the seed\n", q);
  if (seed.status == 0) {
    const vic::Se3 old0 = s.input_cameras[0].T_ck;
    double q4[4];
    RotationToQuat(seed.R_ck, q4);
    for (int j = 0; j < 4; ++j) s.input_cameras[0].T_ck.v[j] = q4[j];                    // the translation stays
    for (size_t c = 1; c < s.input_cameras.size(); ++c)
      s.input_cameras[c].T_ck = Se3Mul(Se3Mul(s.input_cameras[c].T_ck, Se3Inverse(old0)), s.input_cameras[0].T_ck);      // the rig's relative poses stay
    const double angle = 2.0 * std::atan2(std::sqrt(q4[0] * q4[0] + q4[1] * q4[1] + q4[2] * q4[2]), std::fabs(q4[3])) * 180.0 / M_PI;
    std::fprintf(stderr, "I -seed_imu: time offset %.6f ms, R_ck [qx qy qz qw] %.9f %.9f %.9f %.9f (%.3f degrees from identity), gyro bias %.6g %.6g %.6g, "
                         "gravity %.6g %.6g, rms / signal %.4f, %d intervals (%d of %zu frames with a rotation)\n",
                 1e3 * seed.time_offset, q4[0], q4[1], q4[2], q4[3], angle, seed.gyro_bias[0], seed.gyro_bias[1], seed.gyro_bias[2], seed.g_dir[0], seed.g_dir[1],
                 seed.rms / seed.signal, seed.count, n_ok, n_frames);
    if (seed.rms > 0.5 * seed.signal)
      std::fprintf(stderr, "W -seed_imu: the camera's rates and the gyro's explain each other badly (rms / signal %.2f above 0.5): too little rotation about two axes?\n", seed.rms / seed.signal);
  } else if (seed.status > 0) {
    const char* why = seed.status == 1 ? "too few frame intervals with a rate inside the log" : seed.status == 2 ? "the best offset lies on the edge of -seed_imu_range" : "a result is not finite";
    std::fprintf(stderr, "W -seed_imu: no seed (%s; %d of %zu frames with a rotation); starting without it\n", why, n_ok, n_frames);
  }
  return true;
}

// ---- one calibrator per GPU; frames sharded contiguously, the library's own RCCL communicator does the per-iteration
// all-reduces (-gpus 1: plain single-device run, no communicator) -----------------------------------------------------
// from: the result a round of -dot_bias_rounds starts from (cameras, frame poses and velocities, biases, scale factors, gravity, time offset; the
// optimisation flags of -has_initial_guess), instead of the input cameras and the PnP seeds
static bool LoadCalibrators(Run& s, int* rc, const Restart* from = nullptr) {
  const int n_gpus = std::max(1, (int)FlagInt("gpus"));
  const size_t n_cam = s.channels.size(), n_frames = s.frame_ids.size();
  const bool guess = from ? true : FlagBool("has_initial_guess");
  if ((size_t)n_gpus * 2 > n_frames) return Stop(rc, 1, "F -gpus %d needs at least %d frames\n", n_gpus, 2 * n_gpus);
  s.cals.resize((size_t)n_gpus);
  for (int r = 0; r < n_gpus; ++r) {
    try { s.cals[r].reset(new vic::ViCalibrator(Device() + r)); }
    catch (const std::exception& e) { return Stop(rc, 3, "F %s (device %d)\n", e.what(), Device() + r); }
  }
  long n_obs = 0; int seeded = 0;
  s.rank_corners.resize((size_t)n_gpus);
  for (int r = 0; r < n_gpus; ++r) {
    vic::ViCalibrator& cal = *s.cals[r];
    cal.SetSigmas(FlagDouble("gyro_sigma"), FlagDouble("accel_sigma"));                     // vicalib-engine.cc:301-303
    const double zeros[6] = {0, 0, 0, 0, 0, 0}, ones[6] = {1, 1, 1, 1, 1, 1};
    cal.SetBiases(zeros); cal.SetScaleFactor(ones);
    cal.FixCameraIntrinsics(!FlagBool("calibrate_intrinsics"));                            // vicalib-task.cc:128
    for (const vic::CameraAndPose& c : from ? from->cameras : s.input_cameras)
      if (cal.AddCamera(c) < 0) return Stop(rc, 1, "F AddCamera failed (model %s, %zu parameters)\n", ModelName(c.model), c.params.size());
    // every shard gets the whole IMU stream: its last block reaches into the next shard's first frame
    if (s.have_imu && !s.imu.time.empty() && cal.AddImuMeasurements((int)s.imu.time.size(), s.imu.gyro.data(), s.imu.accel.data(), s.imu.time.data()) != VC_OK)
      return Stop(rc, 1, "F IMU measurements rejected\n");
    const size_t lo = n_frames * (size_t)r / (size_t)n_gpus, hi = n_frames * (size_t)(r + 1) / (size_t)n_gpus;
    std::map<long, int> frame_index;
    vic::Se3 placeholder; placeholder.v = {{0, 0, 0, 1, 0, 0, 1000}};                       // vicalib-task.cc:241-244
    for (size_t k = lo; k < hi; ++k) frame_index[s.frame_ids[k]] = cal.AddFrame(placeholder, FrameTime(s.channels, s.frame_ids[k]) + s.image_time_offset);
    std::vector<double> pw, pc;
    for (size_t c = 0; c < n_cam; ++c)
      for (const auto& kv : DetectionsByFrame(s.channels[c], frame_index, s.grid_w * s.grid_h)) {
        pw.clear(); pc.clear();
        AppendCorners(kv.second, &pw, &pc);
        if (FlagBool("output_conics") && !from && !s.quiet_load)
          for (const Detection* d : kv.second) std::printf("%ld,%d,%.10g,%.10g,%.10g,%.10g,%.10g\n", d->frame, d->dot, d->u, d->v, d->X, d->Y, d->Z);
        cal.AddObservations(kv.first, c, (int)kv.second.size(), pw.data(), pc.data());
        if (s.want_report) s.rank_corners[r].insert(s.rank_corners[r].end(), kv.second.begin(), kv.second.end());
        n_obs += (long)kv.second.size();
      }
    if (from) {
      for (size_t k = lo; k < hi; ++k) cal.SetFramePose((int)(k - lo), from->frames[k].t_wp_);
      std::vector<double> v_w;
      for (size_t k = lo; k < hi; ++k) v_w.insert(v_w.end(), from->frames[k].v_w_.begin(), from->frames[k].v_w_.end());
      cal.SetBiases(from->biases.data()); cal.SetScaleFactor(from->scale_factor.data()); cal.SetTimeOffset(from->time_offset);
      if (vc_set_frame_velocities(cal.handle(), v_w.data(), (int)(hi - lo)) != VC_OK) return Stop(rc, 1, "F the frame velocities of the result were rejected\n");
      if (s.calibrate_imu && vc_set_gravity(cal.handle(), from->gravity.data()) != VC_OK) return Stop(rc, 1, "F the gravity of the result was rejected\n");
    } else if (s.imu_seed.status == 0) {                                                   // -seed_imu: the same start on every rank
      const double b[6] = {s.imu_seed.gyro_bias[0], s.imu_seed.gyro_bias[1], s.imu_seed.gyro_bias[2], 0, 0, 0};
      cal.SetTimeOffset(s.imu_seed.time_offset); cal.SetBiases(b);
      if (vc_set_gravity(cal.handle(), s.imu_seed.g_dir) != VC_OK) return Stop(rc, 1, "F the gravity seed was rejected\n");
    }
    cal.SetPnPRansac((int)FlagInt("pnp_ransac_its"), FlagDouble("pnp_ransac_tol"));
    cal.SetPnPDevice(FlagBool("pnp_device"));
    if (!from) seeded += cal.InitFramePosesPnP();
    // ---- VicalibTask::Start(has_initial_guess) (vicalib-task.cc:226-234) + flags read inside the calibrator ---------
    cal.SetOptimizationFlags(guess, guess && s.calibrate_imu, !guess, FlagBool("find_time_offset"));
    cal.SetFunctionTolerance(FlagDouble("function_tolerance"));
    cal.SetMaxIters((int)FlagInt("max_iters"));
    cal.SetCalibrateImu(s.calibrate_imu);
    cal.SetRemoveOutliers(FlagBool("remove_outliers"), FlagDouble("outlier_threshold"));
  }
  if (from || s.quiet_load) return true;
  std::fprintf(stderr, "I %zu cameras, %zu frames on %d GPU(s) (%d with a PnP seed), %ld corner observations, %zu IMU samples\n", n_cam, n_frames, n_gpus, seeded, n_obs, s.imu.time.size());
  return true;
}

// ncclCommInitRank is collective: every rank joins on a thread of its own
static bool SetupCommunicator(Run& s, int* rc) {
  const int n_gpus = (int)s.cals.size();
  if (n_gpus < 2) return true;
  char id[128];
  if (vc_rccl_unique_id(id) != VC_OK) return Stop(rc, 3, "F RCCL is not available (librccl.so)\n");
  std::vector<int> st((size_t)n_gpus, 0);
  std::vector<std::thread> th;
  for (int r = 0; r < n_gpus; ++r) th.emplace_back([&, r] { st[r] = vc_set_shard_rccl(s.cals[r]->handle(), r, n_gpus, id); });
  for (std::thread& t : th) t.join();
  for (int r = 0; r < n_gpus; ++r) if (st[r] != VC_OK) return Stop(rc, 3, "F RCCL communicator setup failed on rank %d (%d)\n", r, st[r]);
  return true;
}

// Start, the 30 ms polling loop (vicalib-engine.cc:376-431), Stop
static void Solve(Run& s) {
  vic::ViCalibrator& cal = *s.cals[0];
  const auto t0 = std::chrono::steady_clock::now();
  for (auto& c : s.cals) c->Start();
  unsigned last_iters = ~0u;
  auto any_running = [&] { for (auto& c : s.cals) if (c->IsRunning()) return true; return false; };
  while (any_running()) {
    const unsigned it = cal.GetNumIterations();
    if (it != last_iters) { std::fprintf(stderr, "I iteration %u  mse %.6g\n", it, cal.MeanSquaredError()); last_iters = it; }
    std::this_thread::sleep_for(std::chrono::milliseconds(30));
  }
  for (auto& c : s.cals) c->Stop();
  s.secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  for (auto& c : s.cals) for (size_t i = 0; i < c->NumFrames(); ++i) s.all_frames.push_back(c->GetFrame(i));
}

// ---- what the rounds of -dot_bias_rounds and -refine_target_rounds share: the result as a start, and the calibrator rebuilt from it (with whatever the
// round changed in the detections) and solved again
static Restart RestartAtResult(Run& s) {
  Restart at;
  vic::ViCalibrator& cal = *s.cals[0];
  at.cameras = CamerasAtResult(cal, s.input_cameras);
  at.frames = s.all_frames;
  at.biases = cal.GetBiases(); at.scale_factor = cal.GetScaleFactor(); at.gravity = cal.GetGravity(); at.time_offset = cal.time_offset();
  return at;
}
static bool RebuildAndSolve(Run& s, const Restart& at, int* rc) {
  s.cals.clear(); s.rank_corners.clear(); s.all_frames.clear();
  if (!LoadCalibrators(s, rc, &at)) return false;
  Solve(s);
  return true;
}

// ---- one round of -dot_bias_rounds: the bias of every calibrated observation predicted at the result (its cameras and T_ck, the frames' T_wk) in
// one batch on -device, subtracted from the ORIGINAL detections (nothing accumulates round over round), the calibrator rebuilt from the result
// and solved again.  An observation whose bias cannot be predicted (status != 0) keeps its original pixel.
static bool DotBiasRound(Run& s, int round, int* rc) {
  const size_t n_cam = s.channels.size();
  const Restart at = RestartAtResult(s);
  const std::vector<double> rmse_before = s.cals[0]->GetCameraProjRMSE();
  if (s.original_uv.empty()) {
    s.original_uv.resize(n_cam);
    for (size_t c = 0; c < n_cam; ++c)
      for (const Detection& d : s.channels[c].det) s.original_uv[c].insert(s.original_uv[c].end(), {d.u, d.v});
  }
  const std::map<long, int> fit_index = FrameIndex(s.frame_ids);
  std::vector<int> view_model, view_off(1, 0), obs_cam;
  std::vector<double> view_K, view_T, pw, radius;
  std::vector<Detection*> obs;
  for (size_t c = 0; c < n_cam; ++c)
    for (const auto& kv : DetectionsByFrame(s.channels[c], fit_index, s.grid_w * s.grid_h)) {
      const vic::Se3 T_cw = Se3Mul(at.cameras[c].T_ck, Se3Inverse(at.frames[(size_t)kv.first].t_wp_));
      view_model.push_back(at.cameras[c].model);
      for (size_t j = 0; j < 10; ++j) view_K.push_back(j < at.cameras[c].params.size() ? at.cameras[c].params[j] : 0.0);
      view_T.insert(view_T.end(), T_cw.v.begin(), T_cw.v.end());
      for (const Detection* d : kv.second) {
        pw.insert(pw.end(), {d->X, d->Y, d->Z});
        radius.push_back((size_t)d->dot < s.dot_radius.size() && d->dot >= 0 ? s.dot_radius[(size_t)d->dot] : 0.0);
        obs.push_back(const_cast<Detection*>(d)); obs_cam.push_back((int)c);          // (an element of s.channels[c].det, which this run owns)
      }
      view_off.push_back((int)obs.size());
    }
  vic::DotBiasResult db;
  try { db = vic::DotBiasBatch(Device(), view_model, view_K, view_T, view_off, pw, radius); }
  catch (const std::exception& e) { return Stop(rc, 3, "F -dot_bias_rounds: %s (device %d)\n", e.what(), Device()); }
  std::vector<double> sum2(n_cam, 0.0), worst(n_cam, 0.0);
  std::vector<long> count(n_cam, 0), refused(n_cam, 0);
  s.dot_bias_rows.clear();
  for (size_t i = 0; i < obs.size(); ++i) {
    Detection* d = obs[i];
    const size_t c = (size_t)obs_cam[i], k = (size_t)(d - s.channels[c].det.data());
    const bool ok = db.status[i] == 0;
    const double bu = ok ? db.bias[2 * i] : 0.0, bv = ok ? db.bias[2 * i + 1] : 0.0;
    d->u = s.original_uv[c][2 * k] - bu; d->v = s.original_uv[c][2 * k + 1] - bv;
    ++count[c];
    if (ok) { sum2[c] += bu * bu + bv * bv; worst[c] = std::max(worst[c], std::sqrt(bu * bu + bv * bv)); } else ++refused[c];
    s.dot_bias_rows.push_back(Run::DotBiasRow{d->frame, (int)c, d->dot, bu, bv, ok ? db.radius_px[i] : 0.0, db.status[i]});
  }
  if (!RebuildAndSolve(s, at, rc)) return false;
  const std::vector<double> rmse_after = s.cals[0]->GetCameraProjRMSE();
  long refused_all = 0;
  for (size_t c = 0; c < n_cam; ++c) {
    const long used = count[c] - refused[c];
    std::fprintf(stderr, "I dot bias round %d, camera %zu: bias rms %.6f px, max %.6f px over %ld observations, %ld without a prediction, RMSE %.6g -> %.6g px\n", round, c,
                 used > 0 ? std::sqrt(sum2[c] / used) : 0.0, worst[c], count[c], refused[c], rmse_before[c], rmse_after[c]);
    refused_all += refused[c];
  }
  if (refused_all > 0) std::fprintf(stderr, "W dot bias round %d: %ld observations keep their original pixel (no bias could be predicted: see the status column of dot_bias.csv with -report_dir)\n", round, refused_all);
  return true;
}
// dot_bias.csv of the last round, beside the residual report
static void WriteDotBiasCsv(const Run& s) {
  const std::string dir = FlagString("report_dir");
  (void)mkdir(dir.c_str(), 0777);
  FILE* f = std::fopen((dir + "/dot_bias.csv").c_str(), "w");
  if (!f) { std::fprintf(stderr, "E cannot write dot_bias.csv into %s\n", dir.c_str()); return; }
  std::fprintf(f, "frame,camera,dot,bu,bv,radius_px,status\n");
  for (const Run::DotBiasRow& r : s.dot_bias_rows) std::fprintf(f, "%ld,%d,%d,%.10g,%.10g,%.10g,%d\n", r.frame, r.cam, r.dot, r.bu, r.bv, r.radius_px, r.status);
  std::fclose(f);
}

// ---- -target_points / -refine_target_rounds: the target by dot id.  nominal = what the detections say (the grid); points = nominal, or the rows of
// -target_points, which every detection's p_w is then taken from.
static void TargetIntoDetections(Run& s) {
  for (Channel& ch : s.channels)
    for (Detection& d : ch.det)
      if (d.dot >= 0 && (size_t)d.dot < s.target_seen.size()) { d.X = s.target_points[3 * (size_t)d.dot]; d.Y = s.target_points[3 * (size_t)d.dot + 1]; d.Z = s.target_points[3 * (size_t)d.dot + 2]; }
}
static bool TargetTables(Run& s, int* rc) {
  const size_t P = (size_t)s.grid_w * (size_t)s.grid_h;
  s.target_nominal.assign(3 * P, 0.0); s.target_seen.assign(P, 0); s.target_corners.assign(P, 0); s.target_status.assign(P, 1);
  for (const Channel& ch : s.channels)
    for (const Detection& d : ch.det)
      if (d.dot >= 0 && (size_t)d.dot < P && !s.target_seen[(size_t)d.dot]) {
        s.target_seen[(size_t)d.dot] = 1;
        s.target_nominal[3 * (size_t)d.dot] = d.X; s.target_nominal[3 * (size_t)d.dot + 1] = d.Y; s.target_nominal[3 * (size_t)d.dot + 2] = d.Z;
      }
  s.target_points = s.target_nominal;
  const std::string file = FlagString("target_points");
  if (file.empty()) return true;
  FILE* f = std::fopen(file.c_str(), "r");
  if (!f) return Stop(rc, 1, "F cannot read -target_points %s\n", file.c_str());
  char line[512];
  long rows = 0;
  while (std::fgets(line, sizeof(line), f)) {
    int dot = -1; double x, y, z;
    if (std::sscanf(line, "%d,%lf,%lf,%lf", &dot, &x, &y, &z) != 4) continue;      // (the header)
    if (dot < 0 || (size_t)dot >= P || !std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) { std::fclose(f); return Stop(rc, 1, "F -target_points %s: dot %d is not a dot of the %d x %d target or its position is not finite\n", file.c_str(), dot, s.grid_w, s.grid_h); }
    s.target_points[3 * (size_t)dot] = x; s.target_points[3 * (size_t)dot + 1] = y; s.target_points[3 * (size_t)dot + 2] = z;
    ++rows;
  }
  std::fclose(f);
  if (rows == 0) return Stop(rc, 1, "F -target_points %s holds no dot\n", file.c_str());
  std::fprintf(stderr, "I target: %ld dots from %s\n", rows, file.c_str());
  return true;      // (the detections keep the nominal target until the frames have their pose seeds: SeedThenMeasuredTarget)
}
// -target_points: the pose seed is a PLANAR PnP and refuses a target that is not flat, so the calibrators are loaded and seeded with the nominal
// target first, then loaded again with the measured one and given those seeds.  Everything else is the fresh start it would have been.
static bool SeedThenMeasuredTarget(Run& s, int* rc) {
  std::vector<std::vector<vic::Se3>> seeds(s.cals.size());
  for (size_t r = 0; r < s.cals.size(); ++r)
    for (size_t i = 0; i < s.cals[r]->NumFrames(); ++i) seeds[r].push_back(s.cals[r]->GetFrame(i).t_wp_);
  TargetIntoDetections(s);
  s.cals.clear(); s.rank_corners.clear();
  s.quiet_load = true;
  const bool ok = LoadCalibrators(s, rc);
  s.quiet_load = false;
  if (!ok) return false;
  for (size_t r = 0; r < s.cals.size(); ++r)
    for (size_t i = 0; i < seeds[r].size(); ++i) s.cals[r]->SetFramePose((int)i, seeds[r][i]);
  return true;
}
// one round of -refine_target_rounds: the step of DESIGN 4.22 at the result over all calibrated observations, the calibrator rebuilt from the result with
// the refined target, solved again.  A singular result or a point that stayed unrefined: a W line, the round is skipped and the target kept.
static bool RefineTargetRound(Run& s, int round, int* rc) {
  const size_t n_cam = s.channels.size(), P = s.target_seen.size();
  const Restart at = RestartAtResult(s);
  const std::vector<double> rmse_before = s.cals[0]->GetCameraProjRMSE();
  std::vector<int> model, flags, tile_frame, tile_cam, point_id;
  std::vector<double> params, T_ck, T_wk, p_c;
  std::vector<long long> tile_off(1, 0);
  for (size_t c = 0; c < n_cam; ++c) {
    model.push_back(at.cameras[c].model);
    for (size_t j = 0; j < 10; ++j) params.push_back(j < at.cameras[c].params.size() ? at.cameras[c].params[j] : 0.0);
    T_ck.insert(T_ck.end(), at.cameras[c].T_ck.v.begin(), at.cameras[c].T_ck.v.end());
    flags.push_back((c == 0 ? 0 : 3) | (FlagBool("calibrate_intrinsics") ? 4 : 0));      // (the calibrator's layout without an IMU: camera 0 carries the rig)
  }
  for (const vic::VicalibFrame& fr : at.frames) T_wk.insert(T_wk.end(), fr.t_wp_.v.begin(), fr.t_wp_.v.end());
  const std::map<long, int> fit_index = FrameIndex(s.frame_ids);
  for (size_t c = 0; c < n_cam; ++c)
    for (const auto& kv : DetectionsByFrame(s.channels[c], fit_index, s.grid_w * s.grid_h)) {
      tile_frame.push_back(kv.first); tile_cam.push_back((int)c);
      for (const Detection* d : kv.second) { point_id.push_back(d->dot); p_c.push_back(d->u); p_c.push_back(d->v); }
      tile_off.push_back((long long)point_id.size());
    }
  const double sigma = FlagDouble("refine_target_sigma");
  vic::TargetRefineResult tr;
  try { tr = vic::TargetRefineBatch(Device(), model, params, T_ck, flags, T_wk, tile_frame, tile_cam, tile_off, point_id, p_c, s.target_points, s.target_nominal, 1.0 / (sigma * sigma)); }
  catch (const std::exception& e) { return Stop(rc, 3, "F -refine_target_rounds: %s (device %d)\n", e.what(), Device()); }
  int refined = 0, unobserved = 0;
  for (size_t p = 0; p < P; ++p) (tr.point_status[p] == 0 ? refined : unobserved) += 1;
  s.target_corners = tr.point_corners; s.target_status = tr.point_status;
  if (tr.status != 0 || unobserved > 0) {
    std::fprintf(stderr, "W target round %d skipped, the target is kept: %s (%d of %zu points without a usable corner)\n", round,
                 tr.status != 0 ? "the system is singular" : "a point stayed unrefined", unobserved, P);
    return true;
  }
  double sum2[3] = {0, 0, 0}, worst = 0.0;
  for (size_t p = 0; p < P; ++p) {
    double n2 = 0.0;
    for (int a = 0; a < 3; ++a) { const double d = tr.refined[3 * p + a] - s.target_nominal[3 * p + a]; sum2[a] += d * d; n2 += d * d; }
    worst = std::max(worst, std::sqrt(n2));
  }
  s.target_points = tr.refined;
  TargetIntoDetections(s);
  if (!RebuildAndSolve(s, at, rc)) return false;
  const std::vector<double> rmse_after = s.cals[0]->GetCameraProjRMSE();
  std::string rm;
  for (size_t c = 0; c < n_cam; ++c) { char b[96]; std::snprintf(b, sizeof(b), "%s%.6g -> %.6g", c ? ", " : "", rmse_before[c], rmse_after[c]); rm += b; }
  std::fprintf(stderr, "I target round %d: offset rms %.4f %.4f %.4f mm, max %.4f mm, %d points refined, %d unobserved, gauge rank %d, RMSE %s px\n", round,
               1e3 * std::sqrt(sum2[0] / P), 1e3 * std::sqrt(sum2[1] / P), 1e3 * std::sqrt(sum2[2] / P), 1e3 * worst, refined, unobserved, tr.gauge_rank, rm.c_str());
  return true;
}
static void WriteTargetCsv(Run& s) {
  const std::string file = FlagString("refine_target_output");
  FILE* f = std::fopen(file.c_str(), "w");
  if (!f) { std::fprintf(stderr, "E cannot write %s\n", file.c_str()); s.incomplete.push_back("-refine_target_output: the file is"); return; }
  std::fprintf(f, "dot,x,y,z,nx,ny,nz,corners,status\n");
  for (size_t p = 0; p < s.target_seen.size(); ++p)
    std::fprintf(f, "%zu,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%d,%d\n", p, s.target_points[3 * p], s.target_points[3 * p + 1], s.target_points[3 * p + 2], s.target_nominal[3 * p],
                 s.target_nominal[3 * p + 1], s.target_nominal[3 * p + 2], s.target_corners[p], s.target_status[p]);
  std::fclose(f);
}

// ---- Finish + PrintResults (vicalibrator.h:536-544) ------------------------------------------------------------------
static void PrintResults(Run& s) {
  vic::ViCalibrator& cal = *s.cals[0];
  s.rmse = cal.GetCameraProjRMSE();
  std::printf("------------------------------------------\n");
  for (size_t c = 0; c < s.channels.size(); ++c) {
    const vic::CameraAndPose cam = cal.GetCamera(c);
    std::printf("Camera: %zu (%s)\n ", c, ModelName(s.input_cameras[c].model));
    for (double p : cam.params) std::printf(" %.10g", p);
    std::printf("\n  T_ck [qx qy qz qw tx ty tz]:");
    for (double p : cam.T_ck.v) std::printf(" %.10g", p);
    std::printf("\n  reprojection RMSE: %.6g px\n", s.rmse[c]);
  }
  if (s.calibrate_imu) {
    const auto b = cal.GetBiases(), sf = cal.GetScaleFactor(); const auto g = cal.GetGravity();
    std::printf("IMU biases (gyro, accel): %.8g %.8g %.8g  %.8g %.8g %.8g\n", b[0], b[1], b[2], b[3], b[4], b[5]);
    std::printf("IMU scale factors:        %.8g %.8g %.8g  %.8g %.8g %.8g\n", sf[0], sf[1], sf[2], sf[3], sf[4], sf[5]);
    std::printf("gravity direction: %.8g %.8g   time offset: %.9g s\n", g[0], g[1], cal.time_offset());
  }
  std::printf("iterations: %u  mse: %.8g  solve time: %.3f s\n", cal.GetNumIterations(), cal.MeanSquaredError(), s.secs);
  if (!FlagBool("print_covariance")) return;
  int dim = 0;                              // GetSolutionCovariance + its log lines (vicalibrator.h:802-857, :1004-1013)
  const std::vector<double> cov = CovarianceOnEveryRank(s.cals, &dim);
  if (dim > 0) {
    std::printf("Covariance calculated for blocks: %s\nSolution covariance:\n", cal.covariance_names().c_str());
    for (int i = 0; i < dim; ++i) {
      for (int j = 0; j < dim; ++j) std::printf(" %.6e", cov[(size_t)i * dim + j]);
      std::printf("\n");
    }
  } else std::printf("Failed to compute covariance...\n");
}

// ---- residual report (-report_dir, -report_worst): per rank, rows concatenated in frame order, maps summed ----------------------------
static void ResidualReport(Run& s) {
  struct ViewRow { long frame; int cam, count, removed; double rmse, max_err; int worst_dot; };
  const size_t n_cam = s.channels.size(), n_gpus = s.cals.size(), n_frames = s.frame_ids.size();
  const int report_bx = s.report_bx, report_by = s.report_by;
  std::vector<ViewRow> views;
  std::vector<std::vector<double>> maps(n_cam, std::vector<double>((size_t)report_bx * report_by * 4, 0.0));
  const std::string dir = FlagString("report_dir");
  FILE* fc = nullptr; FILE* fi = nullptr;
  bool ok = true;
  if (!dir.empty()) {
    (void)mkdir(dir.c_str(), 0777);
    fc = std::fopen((dir + "/corners.csv").c_str(), "w");
    if (!fc) { std::fprintf(stderr, "E cannot write the report into %s\n", dir.c_str()); ok = false; }
    else std::fprintf(fc, "frame,camera,dot,u,v,ru,rv,removed\n");
  }
  try {
    for (size_t r = 0; r < n_gpus && ok; ++r) {
      vic::ViCalibrator& rc = *s.cals[r];
      rc.ReportCompute(report_bx, report_by);
      const std::vector<const Detection*>& dets = s.rank_corners[r];
      const size_t lo = n_frames * r / n_gpus;                  // (the rank's local frame -> id as in the input)
      const vic::ViCalibrator::ReportViews v = rc.GetReportViews();
      for (size_t i = 0; i < v.frame.size(); ++i) {
        const long wc = (long)v.worst_corner[i];
        views.push_back(ViewRow{s.frame_ids[lo + (size_t)v.frame[i]], v.camera[i], v.count[i], v.removed[i], v.count[i] > 0 ? std::sqrt(v.sum_sq[i] / (2.0 * v.count[i])) : 0.0,
                                v.max_err[i], wc >= 0 ? dets[(size_t)wc]->dot : -1});
      }
      for (size_t c = 0; c < n_cam; ++c) {
        const std::vector<double> m = rc.GetReportErrorMap((int)c, report_bx, report_by);
        for (size_t k = 0; k < m.size(); ++k) maps[c][k] += m[k];
      }
      if (fc) {
        const size_t kSlice = 65536;
        std::vector<double> res(2 * kSlice); std::vector<int> cam(kSlice); std::vector<unsigned char> fl(kSlice);
        for (size_t first = 0; first < dets.size(); first += kSlice) {
          const size_t n = std::min(kSlice, dets.size() - first);
          rc.ReportCorners((long long)first, (long long)n, res.data(), nullptr, cam.data(), fl.data());
          for (size_t k = 0; k < n; ++k) {
            const Detection* d = dets[first + k];
            std::fprintf(fc, "%ld,%d,%d,%.10g,%.10g,%.10g,%.10g,%d\n", d->frame, cam[k], d->dot, d->u, d->v, res[2 * k], res[2 * k + 1], (int)fl[k]);
          }
        }
      }
      const size_t nb = rc.NumReportImuBlocks();
      if (nb > 0 && !dir.empty()) {
        if (!fi) {
          fi = std::fopen((dir + "/imu_blocks.csv").c_str(), "w");
          if (fi) {
            std::fprintf(fi, "frame,time");
            for (int k = 0; k < 9; ++k) std::fprintf(fi, ",whitened%d", k);
            for (int k = 0; k < 9; ++k) std::fprintf(fi, ",unwhitened%d", k);
            std::fprintf(fi, ",flag\n");
          }
        }
        std::vector<double> w(9 * nb), u(9 * nb); std::vector<unsigned char> fl(nb);
        rc.ReportImu(w.data(), u.data(), fl.data());
        for (size_t b = 0; b < nb && fi; ++b) {
          std::fprintf(fi, "%ld,%.9f", s.frame_ids[lo + b], rc.GetFrame(b).time);
          for (int k = 0; k < 9; ++k) std::fprintf(fi, ",%.10g", w[9 * b + k]);
          for (int k = 0; k < 9; ++k) std::fprintf(fi, ",%.10g", u[9 * b + k]);
          std::fprintf(fi, ",%d\n", (int)fl[b]);
        }
      }
    }
  } catch (const std::exception& e) { std::fprintf(stderr, "E residual report failed: %s\n", e.what()); ok = false; }
  if (fc) std::fclose(fc);
  if (fi) std::fclose(fi);
  if (ok && !dir.empty()) {
    if (FILE* f = std::fopen((dir + "/views.csv").c_str(), "w")) {
      std::fprintf(f, "frame,camera,corners,removed,rmse_px,max_px,worst_dot\n");
      for (const ViewRow& v : views) std::fprintf(f, "%ld,%d,%d,%d,%.10g,%.10g,%d\n", v.frame, v.cam, v.count, v.removed, v.rmse, v.max_err, v.worst_dot);
      std::fclose(f);
    }
    for (size_t c = 0; c < n_cam; ++c)
      if (FILE* f = std::fopen((dir + "/error_map_cam" + std::to_string(c) + ".csv").c_str(), "w")) {
        std::fprintf(f, "ix,iy,count,mean_ru,mean_rv,rms\n");
        for (int iy = 0; iy < report_by; ++iy) for (int ix = 0; ix < report_bx; ++ix) {
          const double* m = &maps[c][((size_t)iy * report_bx + ix) * 4];
          const double n = m[0];
          std::fprintf(f, "%d,%d,%.0f,%.10g,%.10g,%.10g\n", ix, iy, n, n > 0 ? m[1] / n : 0.0, n > 0 ? m[2] / n : 0.0, n > 0 ? std::sqrt(m[3] / (2.0 * n)) : 0.0);
        }
        std::fclose(f);
      }
  }
  if (ok && FlagInt("report_worst") > 0)
    for (size_t c = 0; c < n_cam; ++c) {
      std::vector<const ViewRow*> of;
      for (const ViewRow& v : views) if (v.cam == (int)c && v.count > 0) of.push_back(&v);
      std::stable_sort(of.begin(), of.end(), [](const ViewRow* a, const ViewRow* b) { return a->rmse > b->rmse; });
      std::printf("worst views of camera %zu (reprojection RMSE):\n", c);
      for (size_t k = 0; k < of.size() && k < (size_t)FlagInt("report_worst"); ++k)
        std::printf("  frame %ld: rmse %.6g px, max %.6g px at dot %d, %d corners, %d removed\n", of[k]->frame, of[k]->rmse, of[k]->max_err, of[k]->worst_dot, of[k]->count, of[k]->removed);
    }
}

// ---- held-out scoring (-holdout_every): rank 0's calibrator refits the poses of the frames kept out, cameras frozen at the result (the
// shared parameters are identical on every rank), and reports how well the calibration predicts views it has not seen ---------------------
static void ScoreHeldOut(Run& s) {
  vic::ViCalibrator& cal = *s.cals[0];
  const size_t n_cam = s.channels.size();
  try {
    const std::map<long, int> held_index = FrameIndex(s.held_ids);
    std::vector<int> tile_frame, tile_cam, point_id;
    std::vector<long long> tile_off(1, 0);
    std::vector<double> points, pc;
    std::vector<const Detection*> dets;
    for (size_t c = 0; c < n_cam; ++c)
      for (const auto& kv : DetectionsByFrame(s.channels[c], held_index, s.grid_w * s.grid_h)) {
        AppendCorners(kv.second, &points, &pc);
        for (const Detection* d : kv.second) { point_id.push_back((int)dets.size()); dets.push_back(d); }
        tile_frame.push_back(kv.first); tile_cam.push_back((int)c); tile_off.push_back((long long)dets.size());
      }
    // (a held-out frame nobody detected the target in still is a frame of the set)
    tile_frame.push_back((int)s.held_ids.size() - 1); tile_cam.push_back(0); tile_off.push_back((long long)dets.size());
    cal.HoldoutClear();
    cal.HoldoutAddTiles((int)tile_frame.size(), tile_frame.data(), tile_cam.data(), tile_off.data(), points.data(), (int)dets.size(), point_id.data(), pc.data());
    cal.HoldoutCompute(nullptr, 0);
    const vic::ViCalibrator::HoldoutFrames hf = cal.GetHoldoutFrames();
    if (s.select.k > 0) {
      SelectHeld& sh = s.select_held;
      sh.tile_frame = tile_frame; sh.tile_cam = tile_cam; sh.tile_off = tile_off; sh.point_id = point_id; sh.points = points;
      sh.status = hf.status;
      for (const vic::Se3& T : hf.T_wk) sh.T_wk.insert(sh.T_wk.end(), T.data(), T.data() + 7);
    }
    const vic::ViCalibrator::HoldoutViews hv = cal.GetHoldoutViews();
    const vic::ViCalibrator::HoldoutCameraRmse hr = cal.GetHoldoutCameraRmse();
    for (size_t c = 0; c < n_cam; ++c) {
      int k = 0;
      for (size_t i = 0; i < hv.frame.size(); ++i) k += (hv.camera[i] == (int)c && hf.status[hv.frame[i]] <= 1) ? 1 : 0;
      std::printf("Camera %zu: fitted RMSE %.6g px, held-out RMSE %.6g px over %d views, %lld corners\n", c, s.rmse[c], hr.rmse[c], k, hr.count[c]);
    }
    int by_status[5] = {0, 0, 0, 0, 0};
    for (int st : hf.status) if (st >= 0 && st < 5) ++by_status[st];
    std::printf("held-out frames: %zu (every %d.)", s.held_ids.size(), s.holdout_every);
    for (int st = 0; st < 5; ++st) if (by_status[st] || st == 0) std::printf("%s %d %s", st ? "," : ":", by_status[st], HoldoutStatusName(st));
    std::printf("\n");
    const std::string dir = FlagString("report_dir");
    if (dir.empty()) return;
    (void)mkdir(dir.c_str(), 0777);
    if (FILE* f = std::fopen((dir + "/holdout_views.csv").c_str(), "w")) {
      std::fprintf(f, "frame,camera,corners,rmse_px,max_px,status,iterations\n");
      for (size_t i = 0; i < hv.frame.size(); ++i)
        std::fprintf(f, "%ld,%d,%d,%.10g,%.10g,%s,%d\n", s.held_ids[(size_t)hv.frame[i]], hv.camera[i], hv.count[i],
                     hv.count[i] > 0 ? std::sqrt(hv.sum_sq[i] / (2.0 * hv.count[i])) : 0.0, hv.max_err[i], HoldoutStatusName(hf.status[hv.frame[i]]), hf.iterations[hv.frame[i]]);
      std::fclose(f);
    } else std::fprintf(stderr, "E cannot write the held-out scores into %s\n", dir.c_str());
    if (FILE* f = std::fopen((dir + "/holdout_corners.csv").c_str(), "w")) {
      std::fprintf(f, "frame,camera,dot,u,v,ru,rv\n");
      const size_t kSlice = 65536;
      std::vector<double> res(2 * kSlice); std::vector<int> cam(kSlice);
      for (size_t first = 0; first < dets.size(); first += kSlice) {
        const size_t n = std::min(kSlice, dets.size() - first);
        cal.HoldoutCorners((long long)first, (long long)n, res.data(), nullptr, cam.data());
        for (size_t k = 0; k < n; ++k) {
          const Detection* d = dets[first + k];
          std::fprintf(f, "%ld,%d,%d,%.10g,%.10g,%.10g,%.10g\n", d->frame, cam[k], d->dot, d->u, d->v, res[2 * k], res[2 * k + 1]);
        }
      }
      std::fclose(f);
    }
  } catch (const std::exception& e) { std::fprintf(stderr, "E held-out scoring failed: %s\n", e.what()); }
}

// ---- the outputs behind WriteCalibration.  Each is one entry: whether it was asked for, the step (false: it failed, why is in *err), whether an
// exception of the step counts as its failure (else it ends the program, as ever), the words of its "E ... failed:" line, the "-flag: the files are"
// of its "incomplete" line, and the place of that line among the nine: they are printed behind the verdict in another order than the steps run.
struct OutputStep { bool on; std::function<bool(std::string*)> run; bool catches; const char* what; const char* incomplete; int place; };
static void PostResultOutputs(Run& s) {
  vic::ViCalibrator& cal = *s.cals[0];
  const std::string& output = FlagString("output");          // (-convert_to, -register_depth and -depthcal_depth re-read the cameras just written)
  std::vector<vic::CameraAndPose> a;
  int dim = 0;
  const OutputStep steps[] = {
    {!FlagString("undistort_dir").empty(), [&](std::string* err) {
       if (!s.from_images) { std::fprintf(stderr, "W -undistort_dir needs image input (-cam file://...): nothing to undistort\n"); return true; }
       return UndistortInputs(cal, s.cam_files, s.input_cameras, s.calibrate_imu, Device(), FlagString("undistort_dir"), FlagDouble("undistort_alpha"), err);
     }, true, "undistortion", "-undistort_dir: the undistorted images are", 0},
    {!FlagString("rectify_dir").empty(), [&](std::string* err) {
       return RectifyOutputs(cal, s.channels, s.frame_ids, s.grid_w * s.grid_h, s.cam_files, s.from_images, s.input_cameras, s.calibrate_imu, Device(), FlagString("rectify_dir"),
                             s.rectify_a, s.rectify_b, FlagDouble("rectify_alpha"), err);
     }, true, "rectification", "-rectify_dir: the rectification's files are", 1},
    {!s.compare_b.empty(), [&](std::string* err) {          // -compare_to: the result (A) against the file (B)
       return CompareRigs(CamerasAtResult(cal, s.input_cameras), s.compare_b, s.compare, Device(), err) == 0;
     }, false, "comparison", "-compare_to: the comparison's files are", 2},
    {!s.uncertainty.dir.empty(), [&](std::string* err) {    // the covariance at the result, mapped per camera
       const std::vector<double> cov = CovarianceOnEveryRank(s.cals, &dim);
       if (cov.empty()) { *err = "the solution covariance cannot be computed"; return false; }
       return UncertaintyOutputs(CamerasAtResult(cal, s.input_cameras), cov, dim, s.rmse, s.uncertainty, Device(), err);
     }, false, "uncertainty map", "-uncertainty_dir: the uncertainty map's files are", 4},
    {!s.stereo_uncertainty.dir.empty(), [&](std::string* err) {      // the covariance at the result, mapped for the pair
       const std::vector<double> cov = CovarianceOnEveryRank(s.cals, &dim);
       if (cov.empty()) { *err = "the solution covariance cannot be computed"; return false; }
       return StereoUncertaintyOutputs(CamerasAtResult(cal, s.input_cameras), cov, dim, s.rmse, s.stereo_uncertainty, Device(), err);
     }, false, "stereo uncertainty map", "-stereo_uncertainty_dir: the stereo uncertainty map's files are", 5},
    {s.select.k > 0, [&](std::string* err) {                // the most informative of the calibrated frames, at the result
       return SelectOutputs(cal, s.frame_ids, s.held_ids, s.select_held, s.select, err);
     }, true, "view selection", "-select_views: the selection's files are", 6},
    {s.converting, [&](std::string* err) {
       return ReadRigFile(output, &a, err) && ConvertRig(output, a, s.convert, s.compare.identity ? &s.compare : nullptr, Device(), err) == 0;
     }, false, "conversion", "-convert_to: the converted rig is", 3},
    {s.reg.on, [&](std::string* err) {
       return ReadRigFile(output, &a, err) && RegisterRig(a, s.reg, Device(), err) == 0;
     }, false, "registration", "-register_depth: the registered images are", 7},
    {s.depthcal.on, [&](std::string* err) {                 // with the poses of the calibration's frames, in their order
       std::vector<std::array<double, 7>> poses;
       for (const vic::VicalibFrame& f : s.all_frames) poses.push_back(f.t_wp_.v);
       return ReadRigFile(output, &a, err) && DepthCalFit(a, poses, "the calibration", s.depthcal, Device(), err) == 0;
     }, false, "depth calibration", "-depthcal_depth: the depth correction is", 8},
  };
  s.incomplete.assign(9, "");
  for (const OutputStep& step : steps) {
    if (!step.on) continue;
    std::string err;
    bool ok = false;
    if (step.catches) {
      try { ok = step.run(&err); } catch (const std::exception& e) { err = e.what(); }
    } else ok = step.run(&err);
    if (ok) continue;
    std::fprintf(stderr, "E %s failed: %s\n", step.what, err.c_str());
    s.incomplete[(size_t)step.place] = step.incomplete;
  }
}

// poses.txt (-print_poses) and poses.csv (-save_poses, vicalib-engine.cc:407-421)
static void WritePoses(const Run& s) {
  if (FILE* f = FlagBool("print_poses") ? std::fopen("poses.txt", "w") : nullptr) {
    for (const vic::VicalibFrame& fr : s.all_frames) { double c[6]; T2Cart(fr.t_wp_.data(), c); std::fprintf(f, "%f\t%f\t%f\t%f\t%f\t%f\n", c[0], c[1], c[2], c[3], c[4], c[5]); }
    std::fclose(f);
  }
  if (FILE* f = FlagBool("save_poses") ? std::fopen("poses.csv", "w") : nullptr) {
    std::fprintf(f, "%% Pose file generated with vicalib.\n%% Each line is the 12 elements from the top 3 rows of a 4x4transformation matrix, printed row major.\n");
    for (const vic::VicalibFrame& fr : s.all_frames) {
      double R[9]; RotationMatrix(fr.t_wp_.data(), R);
      std::fprintf(f, "%.10g %.10g %.10g %.10g     %.10g %.10g %.10g %.10g     %.10g %.10g %.10g %.10g\n", R[0], R[1], R[2], fr.t_wp_.v[4], R[3], R[4], R[5], fr.t_wp_.v[5], R[6], R[7], R[8], fr.t_wp_.v[6]);
    }
    std::fclose(f);
  }
}

// ---- IsSuccessful (vicalib-task.cc:831-856), the verdict, and the exit status: 0, 1 (an output behind the result is incomplete) or 2 (no success)
static int ExitStatus(Run& s) {
  vic::ViCalibrator& cal = *s.cals[0];
  const bool guess = FlagBool("has_initial_guess");
  bool success = true;
  for (size_t c = 0; c < s.channels.size(); ++c)
    if (!(s.rmse[c] <= FlagDouble("max_reprojection_error"))) {
      std::fprintf(stderr, "W Reprojection error of %g was greater than maximum of %g for camera %zu\n", s.rmse[c], FlagDouble("max_reprojection_error"), c);
      success = false;
    }
  if (success && guess) {
    const std::vector<vic::CameraAndPose> now = CamerasAtResult(cal, s.input_cameras);
    for (size_t c = 0; c < now.size() && success; ++c) success = !CameraCalibrationsDiffer(s.input_cameras[c], now[c]);
  }
  if (success && guess) {                        // vicalib-task.cc:852-853 (input_imu_biases_: the calibrator's biases at construction, :129)
    const double input_imu_biases[6] = {0, 0, 0, 0, 0, 0};
    const auto bias_now = cal.GetBiases();
    if (IMUCalibrationDiffer(input_imu_biases, bias_now.data(), FlagString("imu_diff_sense") != "corrected")) success = false;
  }
  std::printf("calibration %s -> %s\n", success ? "succeeded" : "FAILED", FlagString("output").c_str());
  bool any_incomplete = false;
  for (const std::string& what : s.incomplete)
    if (!what.empty()) { std::fprintf(stderr, "E %s incomplete (exit status %d)\n", what.c_str(), success ? 1 : 2); any_incomplete = true; }
  return success ? (any_incomplete ? 1 : 0) : 2;
}

int main(int argc, char** argv) {
  DefineFlags();
  std::string err; int rc = 0;
  const bool parsed = ParseFlags(argc, argv, &err);
  if (err == "help") return Usage(0);
  if (!parsed && !FlagError(&rc, err)) return rc;
  Run s;
  if (!CheckFlags(s, &rc) || !RunStandAloneMode(s, &rc) || !ReadSensors(s, &rc)) return rc;
  if (s.dot_bias_rounds > 0 && !DotRadii(s, &rc)) return rc;
  if (!StartCameras(s, &rc) || !ChooseFrames(s, &rc)) return rc;
  if ((s.refine_rounds > 0 || !FlagString("target_points").empty()) && !TargetTables(s, &rc)) return rc;
  if (FlagBool("seed_focal") && !SeedFocal(s, &rc)) return rc;
  if (FlagString("seed_rig") != "off" && !SeedRig(s, &rc)) return rc;
  s.image_time_offset = InitialTimeOffset(s);
  if (FlagBool("seed_imu") && !SeedImu(s, &rc)) return rc;
  if (!LoadCalibrators(s, &rc)) return rc;
  if (!FlagString("target_points").empty() && !SeedThenMeasuredTarget(s, &rc)) return rc;
  if (!SetupCommunicator(s, &rc)) return rc;
  Solve(s);
  for (int round = 1; round <= s.dot_bias_rounds; ++round)
    if (!DotBiasRound(s, round, &rc)) return rc;
  for (int round = 1; round <= s.refine_rounds; ++round)
    if (!RefineTargetRound(s, round, &rc)) return rc;
  PrintResults(s);
  if (s.refine_rounds > 0) WriteTargetCsv(s);
  if (s.want_report) ResidualReport(s);
  if (s.dot_bias_rounds > 0 && !FlagString("report_dir").empty()) WriteDotBiasCsv(s);
  if (!s.held_ids.empty()) ScoreHeldOut(s);
  s.cals[0]->WriteCameraModels(FlagString("output"));      // WriteCalibration (vicalib-engine.cc:353-372)
  PostResultOutputs(s);
  WritePoses(s);
  return ExitStatus(s);
}
