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
#include <vicalib_amd.hpp>
#include "../vicalib_amd/csrc/vc_holdout_select.hpp"      // which frames -holdout_every keeps out (host arithmetic, no device code)
#include "../vicalib_amd/csrc/vc_allan.hpp"               // the noise model of -allan_imu evaluated at an averaging time (host arithmetic, no device code)

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
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

// ------------------------------------------------------------------------------------------- flags
struct Flag { std::string type, value, help; };
static std::map<std::string, Flag> g_flags;
static void Define(const char* name, const char* type, const char* def, const char* help) { g_flags[name] = Flag{type, def, help}; }
static bool FlagBool(const char* n) { const std::string& v = g_flags.at(n).value; return v == "true" || v == "1" || v == "yes"; }
static double FlagDouble(const char* n) { return std::atof(g_flags.at(n).value.c_str()); }
static long FlagInt(const char* n) { return std::atol(g_flags.at(n).value.c_str()); }
static const std::string& FlagString(const char* n) { return g_flags.at(n).value; }

static void DefineFlags() {
  // vicalib-engine.cc:30-104
  Define("calibrate_imu", "bool", "true", "Calibrate the IMU in addition to the camera.");
  Define("calibrate_intrinsics", "bool", "true", "Calibrate the camera intrinsics as well as the extrinsics.");
  Define("save_poses", "bool", "false", "Save calibrated camera poses when done (poses.csv).");
  Define("exit_vicalib_on_finish", "bool", "true", "Exit when the optimisation finishes.");
  Define("frame_skip", "int32", "0", "Number of frames to skip between constraints.");
  Define("grid_height", "int32", "10", "Height of grid in circles.");
  Define("grid_width", "int32", "19", "Width of grid in circles.");
  Define("grid_spacing", "double", "0.01355", "Distance between circles on grid (m).");
  Define("grid_seed", "int32", "71", "Seed used to generate the grid.");
  Define("has_initial_guess", "bool", "false", "Whether or not the given calibration file has a valid guess.");
  Define("output_conics", "bool", "false", "Echo the detections that were used (frame,dot_id,u,v,X,Y,Z), before the solve; their residuals come from -report_dir.");
  Define("grid_preset", "string", "", "Which grid preset to use: small, large, letter, medium.");
  Define("grid_pattern_file", "string", "", "(image input) large / small pattern of the target: grid_height rows of grid_width 0 / 1 entries (1 = large dot).");
  Define("max_reprojection_error", "double", "0.15", "Maximum allowed reprojection error (pixels).");
  Define("num_vicalib_frames", "int64", "-1", "Number of frames to process before calibration begins (-1: all).");
  Define("print_poses", "bool", "false", "Output poses to poses.txt");
  Define("print_covariance", "bool", "false", "Print the solution covariance of q_ck / p_ck / params (the reference compiles this in with COMPUTE_VICALIB_COVARIANCE).");
  Define("output", "string", "cameras.xml", "Output XML file to write camera models to.");
  Define("output_log_file", "string", "vicalibrator.log", "Calibration result output log file.");
  Define("cam", "string", "", "Camera URI: detections://cam0.csv[,cam1.csv...] or file://dir/cam0_*.pgm[,dir/cam1_*.pgm...] (8-bit PGM images)");
  Define("imu", "string", "", "IMU URI (if available): csv://directory");
  Define("models", "string", "", "Comma-separated list of camera model types: fov, poly2, poly3, rational6, kb4, linear.");
  Define("model_files", "string", "", "Comma-separated list of camera model files to initialise from.");
  Define("max_iters", "int32", "200", "Max iterations.");
  Define("pnp_ransac_its", "int32", "0", "Minimal-sample iterations of the robust pose seed (0: plain PnP, as the reference calls PosePnPRansac).");
  Define("pnp_ransac_tol", "double", "2.0", "Inlier threshold of the robust pose seed, pixels.");
  Define("pnp_device", "bool", "false", "Seed the frame poses with the batched PnP on the GPU instead of the host routine (same seeds to 1e-6).");
  Define("seed_focal", "bool", "false", "Without -model_files: start every camera at the focal length its views of the target give (homographies, on the GPU) instead of 300.");
  Define("seed_focal_radius", "double", "0.5", "Corners used by -seed_focal lie within this fraction of the half diagonal of the image centre (<= 0: the whole image).");
  Define("seed_focal_fit_px", "double", "0", "Views whose homography fits worse than this many pixels rms are left out of -seed_focal (0: off).");
  Define("seed_imu", "bool", "false", "With -imu: start the camera-IMU rotation of camera 0, the time offset, the gyro bias and gravity from the data (camera rates against gyro rates, on the GPU) instead of identity, the streams' first stamps, zero and one accelerometer sample.");
  Define("seed_imu_range", "double", "0.5", "Time offsets searched by -seed_imu: -range ... +range seconds around the start value.");
  Define("seed_imu_step", "double", "0", "Step of that search in seconds (0: the median IMU sample interval).");
  Define("seed_imu_max_gap", "double", "0.5", "Consecutive frames further apart than this many seconds give -seed_imu no rate.");
  Define("seed_imu_min_intervals", "int32", "10", "-seed_imu wants at least this many frame intervals with a rate (at least 3).");
  Define("gyro_sigma", "double", "5.3088444e-5", "Sigma of gyroscope measurements.");
  Define("accel_sigma", "double", "0.001883649", "Sigma of accel measurements.");
  Define("remove_outliers", "bool", "false", "Remove outliers and re-optimise.");
  Define("outlier_threshold", "double", "2.0", "Outlier threshold (x camera RMSE).");
  Define("paused", "bool", "false", "(GUI) ignored.");
  Define("use_only_when_static", "bool", "false", "(sensor front-end) ignored: the detections file already holds the chosen frames.");
  // flags of the sensor / pattern front-end (vicalib-engine.cc:39, :65-77, :88-92, vicalib-task.cc:19): accepted so that an existing
  // command line keeps working, without effect here -- the detections file is what that front-end would have produced
  Define("device_serial", "string", "-1", "(sensor front-end) ignored: serial number of device.");
  Define("scaled_ir_depth_cal", "bool", "false", "(sensor front-end) ignored: produce ir and depth calibration by rescaling RGB.");
  Define("static_accel_threshold", "double", "0.08", "(sensor front-end) ignored: acceleration below which the device counts as static.");
  Define("static_gyro_threshold", "double", "0.04", "(sensor front-end) ignored: angular velocity below which the device counts as static.");
  Define("static_threshold_preset", "int32", "0", "(sensor front-end) ignored: a visual_inertial_calibration::StaticThresholdPreset.");
  Define("use_static_threshold_preset", "bool", "false", "(sensor front-end) ignored: use one of the predefined static thresholds.");
  Define("output_pattern_file", "string", "", "(pattern front-end) ignored: EPS or SVG file to save the calibration pattern.");
  Define("grid_large_rad", "double", "0.00423", "(pattern front-end) ignored: radius of large dots (m).");
  Define("grid_small_rad", "double", "0.00283", "(pattern front-end) ignored: radius of small dots (m).");
  Define("clip_good", "bool", "false", "(sensor front-end) ignored: output proto file of only good tracked images.");
  // vicalib-task.cc:19-51
  Define("find_time_offset", "bool", "true", "Optimize for the time offset between the IMU and images.");
  Define("function_tolerance", "double", "1e-6", "Convergence criterion for the optimizer.");
  Define("max_fx_diff", "double", "10.0", "Maximum fx difference between calibrations.");
  Define("max_fy_diff", "double", "10.0", "Maximum fy difference between calibrations.");
  Define("max_cx_diff", "double", "10.0", "Maximum cx difference between calibrations.");
  Define("max_cy_diff", "double", "10.0", "Maximum cy difference between calibrations.");
  Define("max_fov_w_diff", "double", "0.3", "Maximum fov distortion difference between calibrations.");
  Define("max_poly3_diff_k1", "double", "0.1", "Maximum poly3 k1 difference between calibrations.");
  Define("max_poly3_diff_k2", "double", "0.1", "Maximum poly3 k2 difference between calibrations.");
  Define("max_poly3_diff_k3", "double", "0.1", "Maximum poly3 k3 difference between calibrations.");
  Define("max_camera_trans_diff", "double", "0.1", "Maximum camera translation difference between calibrations.");
  Define("max_camera_angle_diff", "double", "0.1", "Maximum camera angle difference (rad) between calibrations.");
  Define("max_imu_gyro_diff", "double", "0.1", "Maximum gyroscope bias difference between calibrations.");
  Define("max_imu_accel_diff", "double", "0.1", "Maximum accelrometer bias difference between calibrations.");
  Define("imu_diff_sense", "string", "reference", "IMUCalibrationDiffer with -has_initial_guess: 'reference' = the comparisons as the reference writes them "
         "(vicalib-task.cc:811-826: a bias difference BELOW the limit counts as differing), 'corrected' = above the limit.");
  Define("use_system_time", "bool", "true", "Use the first (system) column of timestamp.txt; otherwise the second (device).");
  // new: what HAL would have told the reference
  Define("image_width", "int32", "640", "Image width of every channel (HAL reports it in the reference).");
  Define("image_height", "int32", "480", "Image height of every channel.");
  Define("frame_rate", "double", "30", "Frame rate used for timestamps when the detections carry no time column.");
  Define("device", "int32", "0", "HIP device ordinal (first device with -gpus N).");
  Define("gpus", "int32", "1", "Number of GPUs: frames are sharded, one calibrator per device, RCCL all-reduce per iteration.");
  // residual report (vc_report_*): off unless asked for
  Define("report_dir", "string", "", "Directory for the residual report of the result: views.csv, corners.csv, error_map_cam<c>.csv, imu_blocks.csv (empty: none).");
  Define("report_bins", "string", "16x12", "Cells of the report's error maps, WIDTHxHEIGHT, each 1..32.");
  Define("report_worst", "int32", "0", "Print the N views with the largest reprojection RMSE of every camera behind the results (0: none).");
  // held-out scoring (vc_holdout_*): off unless asked for
  Define("holdout_every", "int32", "0", "Keep every Nth of the frames that survive -frame_skip and -num_vicalib_frames out of the calibration and score the result on "
         "them: held-out RMSE per camera behind the results, holdout_views.csv and holdout_corners.csv with -report_dir (0: off; N >= 2).");
  // undistortion of the input images with the result (vc_undistort*): off unless asked for
  Define("undistort_dir", "string", "", "(image input) Directory for the input images undistorted with the result, cam<i>_<name>.pgm, and cameras.xml with the "
         "pinhole cameras they belong to (empty: none).  Its parent must exist; if the images cannot be written the tool says so and exits with status 1.");
  Define("undistort_alpha", "double", "0", "Destination intrinsics of -undistort_dir: 0 = every pixel of an undistorted image is valid ... 1 = every source pixel is kept.");
  // stereo rectification with the result and its consistency check (vc_rectif*): off unless asked for
  Define("rectify_dir", "string", "", "Directory for the stereo rectification of two cameras with the result: cameras.xml (the two rectified pinhole cameras), "
         "stereo_check.csv (row misalignment and metric consistency of the calibration's own matched detections, per frame) and, with image input, the rectified images cam<i>_<name>.pgm.");
  Define("rectify_cams", "string", "0,1", "The two cameras -rectify_dir rectifies: a,b.");
  Define("rectify_alpha", "double", "0", "Destination intrinsics of -rectify_dir: 0 = every pixel of both rectified images is valid ... 1 = every source pixel of both cameras is kept.");
  // two calibrations compared in pixel space (vc_compar*): off unless asked for
  Define("compare_models", "string", "", "a.xml,b.xml: compare the cameras of two rig files, camera by camera, into -compare_dir; needs no -cam, nothing is calibrated.");
  Define("compare_to", "string", "", "b.xml: compare the calibration just computed (A) with the cameras of this rig file (B) into -compare_dir.");
  Define("compare_dir", "string", "", "Directory for compare_cam<i>.csv (x, y, du, dv, flags per lattice sample, at the implied rotation), compare_summary.csv and, with more "
         "than one camera, compare_extrinsics.csv.  Its parent must exist.");
  Define("compare_grid", "string", "64x48", "Lattice of the comparison, GXxGY: 2 ... image width by 2 ... image height, at most 2^22 samples.");
  Define("compare_fit_radius", "double", "0.5", "The implied rotation is fitted over the samples within this fraction of the half-diagonal of the image centre (> 0).");
  Define("compare_rings", "int32", "8", "Rings of equal width in normalised radius in compare_summary.csv, 1 ... 64.");
  // a calibrated camera converted to another camera model (vc_convert*): off unless asked for
  Define("convert_models", "string", "", "in.xml: convert the cameras of this rig file to the models of -convert_to into -convert_output; needs no -cam, nothing is calibrated.");
  Define("convert_to", "string", "", "m[,m...]: target model(s) of the conversion, one for all cameras or one per camera.  Without -convert_models the calibration just computed "
         "is converted.  With -compare_dir the original is also compared with the converted cameras, at the identity rotation.");
  Define("convert_output", "string", "converted.xml", "Rig file of the converted cameras: every camera keeps its pose and size.");
  Define("uncertainty_dir", "string", "", "Directory for uncertainty_cam<i>.csv (x, y, s_uu, s_uv, s_vv, sigma_max, flags per lattice sample: the covariance in px^2 of the projection "
         "shift that the covariance of the intrinsics leaves after the rotation the extrinsics would absorb) and uncertainty_summary.csv, written behind a calibration.");
  Define("uncertainty_grid", "string", "64x48", "Lattice of the uncertainty map, GXxGY: 2 ... image width by 2 ... image height, at most 2^22 samples.");
  Define("uncertainty_fit_radius", "double", "0.5", "The absorbed rotation is fitted over the samples within this fraction of the half-diagonal of the image centre (<= 0: no rotation is removed).");
  Define("uncertainty_rings", "int32", "8", "Rings of equal width in normalised radius in uncertainty_summary.csv, 1 ... 64.");
  Define("uncertainty_noise", "double", "0", "Detection noise in px per coordinate that scales the covariance; 0 = the camera's own reprojection RMSE.");
  Define("stereo_uncertainty_dir", "string", "", "Directory for stereo_uncertainty.csv (depth, x, y, sigma_dv, sigma_d, sigma_Z, flags per lattice sample of the rectified image of the "
         "first camera and depth: what the covariance of the calibration implies for the row misalignment and the disparity in px and for the depth in m) and "
         "stereo_uncertainty_summary.csv, written behind a calibration.  The rectified camera is the one -rectify_dir uses: fitted at -rectify_alpha, of the first camera's size.");
  Define("stereo_uncertainty_cams", "string", "0,1", "The two cameras of -stereo_uncertainty_dir: a,b.");
  Define("stereo_uncertainty_depths", "string", "0.5,1,2,5", "Depths in m of the map, 1 ... 8 of them, each above 0.");
  Define("stereo_uncertainty_grid", "string", "64x48", "Lattice of the stereo uncertainty map, GXxGY: 2 ... image width by 2 ... image height, at most 2^22 samples.");
  Define("stereo_uncertainty_noise", "double", "0", "Detection noise in px per coordinate that scales the covariance; 0 = the mean of the two cameras' reprojection RMSE.");
  Define("select_views", "string", "", "Behind a calibration, select this many of the calibrated frames by greedy D-optimal view selection (the log-determinant of the "
         "information on the shared vision parameters, every frame's pose marginalised) with the result's cameras and poses; needs -select_dir and -gpus 1.");
  Define("select_dir", "string", "", "Directory for selected_views.csv (rank, frame, gain, cum, share), select_frames.csv (frame, status, corners, behind, first-round gain) and, with "
         "-holdout_every, select_holdout.csv (the held-out frames scored as candidates against the calibrated frames as start set).");
  Define("select_prior", "double", "1e-6", "The prior on every scaled shared column that keeps the first log-determinants finite, > 0.");
  Define("select_start", "string", "", "Frames the selection starts from, f0,f1,... (frame numbers of the recording, each one of the calibrated frames).");
  // a depth image registered into another camera of the rig (vc_regist*): off unless asked for
  Define("register_models", "string", "", "rig.xml: register with the cameras of this rig file; needs no -cam, nothing is calibrated.  Without it -register_depth uses the "
         "calibration just computed.");
  Define("register_cams", "string", "0,1", "s,d: the depth camera s and the camera d its depth images are registered into.");
  Define("register_depth", "string", "", "file://glob of the depth images of camera s: 16-bit binary PGM (maxval 65535, big-endian), 0 = no measurement.  Each is written "
         "to -register_dir/<name>.pgm in camera d's pixels, with register_summary.csv (the eight counters per image).");
  Define("register_dir", "string", "", "Directory for the registered images.  Its parent must exist.");
  Define("register_unit", "double", "0.001", "Metres per count of the depth images, in and out (> 0).");
  Define("register_kind", "string", "z", "What a depth value measures: z (distance along the optical axis) or range (distance along the pixel's ray).");
  Define("register_splat", "string", "nearest", "Where a depth pixel lands: nearest (one pixel) or footprint (the rectangle its corners span, for a finer camera d).");
  Define("register_color", "string", "", "file://glob of 8-bit PGM images of camera d, k-th with k-th depth image: each is taken into camera s's pixels as "
         "-register_dir/color_in_depth_<name>.pgm (0 where camera d does not see the surface).");
  Define("register_occlusion_tol", "double", "10", "A depth pixel sees camera d's image where it lies at most this many counts behind the nearest surface there (>= 0).");
  Define("depthcal_models", "string", "", "rig.xml: calibrate the range error of a depth camera of this rig file against the target, from -depthcal_poses and "
         "-depthcal_depth; needs no -cam, nothing is calibrated.  Without it -depthcal_depth uses the calibration's result and the poses of its frames.");
  Define("depthcal_cam", "int32", "0", "The depth camera.");
  Define("depthcal_poses", "string", "", "The frames' poses in the format -save_poses writes; the k-th line belongs to the k-th file of -depthcal_depth in sorted order.");
  Define("depthcal_depth", "string", "", "file://glob of the depth images: 16-bit binary PGM (maxval 65535, big-endian), 0 = no measurement.");
  Define("depthcal_dir", "string", "", "Directory for depth_correction.csv, depthcal_cells.csv and depthcal_frames.csv (fit) or the corrected images and "
         "depthcal_apply.csv (apply).  Its parent must exist.");
  Define("depthcal_apply", "string", "", "depth_correction.csv: correct the images of -depthcal_depth with it and write them to -depthcal_dir under their own names.");
  Define("depthcal_interp", "string", "cell", "The cells' terms of a correction: cell (the pixel's own cell) or bilinear (between cell centres).");
  Define("depthcal_unit", "double", "0.001", "Metres per count of the depth images (> 0).");
  Define("depthcal_kind", "string", "z", "What a depth value measures: z (distance along the optical axis) or range (distance along the pixel's ray).");
  Define("depthcal_bins", "string", "4,3", "bx,by: image cells of the correction, 1..32 each.");
  Define("depthcal_vref", "double", "1000", "A typical value of the working range in counts (> 0); it only centres the arithmetic.");
  Define("depthcal_min_cos", "double", "0.5", "Pixels that see the board at a cosine of incidence below this are dropped (in (0, 1]).");
  Define("depthcal_max_dev", "double", "100", "Pixels whose value differs from the expected one by more than this many counts are dropped (> 0).");
  Define("depthcal_degree", "int32", "2", "Degree of the global polynomial in the value: 0, 1 or 2.");
  Define("depthcal_min_count", "int32", "50", "A cell with fewer pixels gets no term of its own (>= 1).");
  Define("depthcal_min_spread", "double", "0.02", "A cell whose values spread less than this (standard deviation of (v - vref) / vref) gets an offset only (>= 0).");
  Define("depthcal_margin", "double", "0", "The board rectangle is the dot lattice [0, (grid_width - 1) spacing] x [0, (grid_height - 1) spacing] grown by this (m).");
  Define("allan_imu", "string", "", "csv://directory of an IMU log recorded at rest: its Allan deviation, noise terms and the sigmas to calibrate with go into -allan_dir; needs no -cam, nothing is calibrated.");
  Define("allan_dir", "string", "", "Directory for allan.csv and allan_summary.csv of -allan_imu.");
  Define("allan_per_decade", "int32", "20", "Averaging times per decade of the Allan deviation (1 ... 1000).");
  Define("allan_max_fraction", "double", "0.1111111111111111", "The longest averaging time as a fraction of the samples used (in (0, 0.5]; at 1/9 the standard error of a point is 25 %).");
  Define("allan_static_window_s", "double", "1", "Window of the quiet test in seconds (> 0).");
  Define("allan_static_gyro", "double", "0", "The mean angular velocity may change by less than this from one window to the next for a window to count as quiet (<= 0: not tested).");
  Define("allan_static_accel", "double", "0", "The same for the mean acceleration (<= 0: not tested; both off: the whole log is used).");
  Define("convert_grid", "string", "64x48", "Lattice of the conversion, GXxGY: 2 ... image width by 2 ... image height, at most 2^22 samples.");
  Define("convert_fit_radius", "double", "1", "The target model is fitted over the samples within this fraction of the half-diagonal of the image centre (> 0; 1 = the whole image).");
}

static int Usage(int code) {
  std::printf("vicalib (MI355X solver) -- flags (gflags syntax: -flag value, --flag=value, -noflag)\n");
  for (const auto& kv : g_flags) std::printf("  -%-24s (%s) default: %-12s %s\n", kv.first.c_str(), kv.second.type.c_str(), ("\"" + kv.second.value + "\"").c_str(), kv.second.help.c_str());
  return code;
}

static bool ParseFlags(int argc, char** argv, std::string* err) {
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    if (a == "-h" || a == "-help" || a == "--help") { *err = "help"; return false; }
    if (a.size() < 2 || a[0] != '-') { *err = "unexpected argument '" + a + "'"; return false; }
    a = a.substr(a[1] == '-' ? 2 : 1);
    std::string name = a, value; bool has_value = false;
    const size_t eq = a.find('=');
    if (eq != std::string::npos) { name = a.substr(0, eq); value = a.substr(eq + 1); has_value = true; }
    auto it = g_flags.find(name);
    if (it == g_flags.end() && name.compare(0, 2, "no") == 0) {
      auto it2 = g_flags.find(name.substr(2));
      if (it2 != g_flags.end() && it2->second.type == "bool" && !has_value) { it2->second.value = "false"; continue; }
    }
    if (it == g_flags.end()) { *err = "unknown command line flag '" + name + "'"; return false; }
    if (it->second.type == "bool") {
      if (!has_value) { it->second.value = "true"; continue; }
      it->second.value = (value == "true" || value == "1" || value == "yes" || value == "t" || value == "y") ? "true" : "false";
      continue;
    }
    if (!has_value) {
      if (i + 1 >= argc) { *err = "flag '" + name + "' is missing its argument"; return false; }
      value = argv[++i];
    }
    if (it->second.type != "string") {
      char* end = nullptr; std::strtod(value.c_str(), &end);
      if (end == value.c_str() || *end != 0) { *err = "illegal value '" + value + "' specified for " + it->second.type + " flag '" + name + "'"; return false; }
    }
    it->second.value = value;
  }
  return true;
}

// ------------------------------------------------------------------------------------------- inputs
static std::vector<std::string> Split(const std::string& s, char sep) {
  std::vector<std::string> out; std::stringstream ss(s); std::string item;
  while (std::getline(ss, item, sep)) if (!item.empty()) out.push_back(item);
  return out;
}
static std::string StripScheme(const std::string& uri) {
  const size_t p = uri.find("//");
  return p == std::string::npos ? uri : uri.substr(p + 2);
}
static bool ParseNumbers(const std::string& line, std::vector<double>* v) {
  v->clear();
  const char* p = line.c_str();
  while (*p) {
    while (*p == ' ' || *p == '\t' || *p == ',' || *p == ';' || *p == '\r') ++p;
    if (!*p) break;
    char* end = nullptr;
    const double d = std::strtod(p, &end);
    if (end == p) return false;
    v->push_back(d); p = end;
  }
  return !v->empty();
}

struct Detection { long frame; int dot; double u, v, X, Y, Z; };
struct Channel { std::vector<Detection> det; std::map<long, double> frame_time; };

// ---- image channels (vicalib-task.cc:263-330 with files for sensors) ----------------------------------------------------------------
static bool ReadPgm(const std::string& path, int* w, int* h, std::vector<unsigned char>* px, std::string* err) {
  std::ifstream f(path, std::ios::binary);
  if (!f) { *err = "cannot open image " + path; return false; }
  std::string magic; f >> magic;
  if (magic != "P5") { *err = path + ": not a binary PGM (P5)"; return false; }
  auto next_int = [&](long* v) {
    while (true) { f >> std::ws; if (f.peek() == '#') { std::string c; std::getline(f, c); } else break; }
    return (bool)(f >> *v);
  };
  long W = 0, H = 0, M = 0;
  if (!next_int(&W) || !next_int(&H) || !next_int(&M) || W < 1 || H < 1 || M != 255) { *err = path + ": expected an 8-bit PGM header"; return false; }
  f.get();                                          // the single whitespace byte behind the header
  px->resize((size_t)W * H);
  f.read((char*)px->data(), (std::streamsize)px->size());
  if ((size_t)f.gcount() != px->size()) { *err = path + ": truncated image data"; return false; }
  *w = (int)W; *h = (int)H;
  return true;
}
static bool GlobSorted(const std::string& pattern_glob, std::vector<std::string>* files) {
  glob_t g; std::memset(&g, 0, sizeof(g));
  const bool ok = glob(pattern_glob.c_str(), 0, nullptr, &g) == 0 && g.gl_pathc > 0;
  if (ok) files->assign(g.gl_pathv, g.gl_pathv + g.gl_pathc);
  globfree(&g);
  std::sort(files->begin(), files->end());
  return ok;
}
struct TargetSpec { std::vector<int> pattern; int rows = 0, cols = 0; double spacing = 0.0; };
// one camera channel from a glob of images: frame k = k-th file (sorted); detections carry the target dot's index and position
static bool ReadImages(const std::string& pattern_glob, const TargetSpec& tg, int device, Channel* ch, int* width, int* height, std::string* err) {
  std::vector<std::string> files;
  if (!GlobSorted(pattern_glob, &files)) { *err = "no images match " + pattern_glob; return false; }
  vc_detector* det = nullptr;
  std::vector<unsigned char> px;
  const int kMax = 4096;
  std::vector<double> cen(2 * kMax), con(9 * kMax);
  std::vector<int> box(4 * kMax), idx(kMax);
  long placed = 0, skipped = 0;
  for (size_t k = 0; k < files.size(); ++k) {
    int w = 0, h = 0;
    if (!ReadPgm(files[k], &w, &h, &px, err)) { if (det) vc_detector_destroy(det); return false; }
    if (!det) {
      const int rc = vc_detector_create(device, w, h, &det);
      if (rc != VC_OK) { *err = rc == VC_ERR_NO_DEVICE ? "no usable HIP device for the dot detector" : "vc_detector_create failed"; return false; }
      *width = w; *height = h;
    } else if (w != *width || h != *height) { *err = files[k] + ": image size differs from the first image of the channel"; vc_detector_destroy(det); return false; }
    int n = 0, m = 0;
    if (vc_detector_find_conics(det, px.data(), w, cen.data(), con.data(), box.data(), kMax, &n) != VC_OK ||
        vc_target_find(cen.data(), con.data(), n, tg.pattern.data(), tg.rows, tg.cols, idx.data(), &m) != VC_OK) { *err = files[k] + ": detection failed"; vc_detector_destroy(det); return false; }
    if (m == 0) { ++skipped; continue; }                 // "Tracking bad" (vicalib-task.cc:278-281): the frame contributes nothing
    for (int i = 0; i < n; ++i) {
      if (idx[i] < 0) continue;
      const int r = idx[i] / tg.cols, c = idx[i] % tg.cols;
      ch->det.push_back(Detection{(long)k, idx[i], cen[2 * i], cen[2 * i + 1], c * tg.spacing, r * tg.spacing, 0.0});
      ++placed;
    }
  }
  if (det) vc_detector_destroy(det);
  std::fprintf(stderr, "I %s: %zu images, %ld dots associated with the target, %ld images without an unambiguous placement\n", pattern_glob.c_str(), files.size(), placed, skipped);
  return true;
}
static bool ReadDetections(const std::string& path, Channel* ch, std::string* err) {
  std::ifstream f(path);
  if (!f) { *err = "cannot open detections file " + path; return false; }
  std::string line; std::vector<double> v; long ln = 0;
  while (std::getline(f, line)) {
    ++ln;
    if (line.empty() || line[0] == '#' || line[0] == '%') continue;
    if (!ParseNumbers(line, &v)) continue;                    // header / log text between the detection lines
    if (v.size() < 7) { *err = path + ":" + std::to_string(ln) + ": expected frame,dot_id,u,v,X,Y,Z[,time]"; return false; }
    if (v[1] < 0) continue;                                   // unmatched conic (vicalib-task.cc:309-311)
    ch->det.push_back(Detection{(long)v[0], (int)v[1], v[2], v[3], v[4], v[5], v[6]});
    if (v.size() >= 8) ch->frame_time[(long)v[0]] = v[7];
  }
  return true;
}

struct ImuData { std::vector<double> gyro, accel, time; };
static bool ReadColumns(const std::string& path, int min_cols, std::vector<std::vector<double>>* rows, std::string* err) {
  std::ifstream f(path);
  if (!f) { *err = "cannot open " + path; return false; }
  std::string line; std::vector<double> v;
  while (std::getline(f, line)) {
    if (line.empty() || line[0] == '#' || line[0] == '%') continue;
    if (!ParseNumbers(line, &v)) continue;
    if ((int)v.size() < min_cols) { *err = path + ": expected at least " + std::to_string(min_cols) + " columns"; return false; }
    rows->push_back(v);
  }
  return true;
}
static bool ReadImu(const std::string& dir, bool system_time, ImuData* imu, std::string* err) {
  std::vector<std::vector<double>> a, g, t;
  if (!ReadColumns(dir + "/accel.txt", 3, &a, err) || !ReadColumns(dir + "/gyro.txt", 3, &g, err) || !ReadColumns(dir + "/timestamp.txt", 1, &t, err)) return false;
  const size_t n = std::min(a.size(), std::min(g.size(), t.size()));
  double last = -1e300;
  for (size_t i = 0; i < n; ++i) {
    const double ts = (!system_time && t[i].size() > 1) ? t[i][1] : t[i][0];
    if (ts <= last) continue;                                 // the calibrator insists on strictly increasing time (vicalibrator.h:373-378)
    last = ts;
    imu->time.push_back(ts);
    for (int k = 0; k < 3; ++k) { imu->gyro.push_back(g[i][k]); imu->accel.push_back(a[i][k]); }
  }
  return true;
}

static int ModelId(const std::string& type) {     // -models strings (vicalib-engine.cc:203-253) and XML type strings (:210-260)
  if (type == "fov" || type == "calibu_fu_fv_u0_v0_w") return VC_MODEL_FOV;
  if (type == "poly2" || type == "calibu_fu_fv_u0_v0_k1_k2") return VC_MODEL_POLY2;
  if (type == "poly3" || type == "poly" || type == "calibu_fu_fv_u0_v0_k1_k2_k3") return VC_MODEL_POLY3;
  if (type == "kb4" || type == "calibu_fu_fv_u0_v0_kb4") return VC_MODEL_KB4;
  if (type == "linear" || type == "calibu_fu_fv_u0_v0") return VC_MODEL_LINEAR;
  if (type == "rational6" || type == "rational" || type == "calibu_fu_fv_u0_v0_rational6") return VC_MODEL_RATIONAL6;      // vicalib-engine.cc:233-240
  return -1;
}
static const char* ModelName(int id) { static const char* n[] = {"fov", "poly2", "poly3", "kb4", "linear", "rational6"}; return (id >= 0 && id < 6) ? n[id] : "?"; }

static std::string Between(const std::string& s, const std::string& a, const std::string& b, size_t from = 0) {
  const size_t p = s.find(a, from); if (p == std::string::npos) return "";
  const size_t q = s.find(b, p + a.size()); if (q == std::string::npos) return "";
  return s.substr(p + a.size(), q - p - a.size());
}
// first <camera_model> of a calibu rig XML (the reference takes rig->cameras_[0], pose ignored: vicalib-engine.cc:190-197)
static bool ReadModelFile(const std::string& path, vic::CameraAndPose* cam, std::string* err) {
  std::ifstream f(path);
  if (!f) { *err = "cannot open model file " + path; return false; }
  std::stringstream ss; ss << f.rdbuf();
  const std::string s = ss.str();
  const std::string head = Between(s, "<camera_model", ">");
  cam->model = ModelId(Between(head, "type=\"", "\""));
  if (cam->model < 0) { *err = path + ": unsupported camera model type '" + Between(head, "type=\"", "\"") + "'"; return false; }
  std::vector<double> v;
  if (ParseNumbers(Between(s, "<width>", "</width>"), &v)) cam->width = (int)v[0];
  if (ParseNumbers(Between(s, "<height>", "</height>"), &v)) cam->height = (int)v[0];
  std::string p = Between(s, "<params>", "</params>");
  std::replace(p.begin(), p.end(), '[', ' '); std::replace(p.begin(), p.end(), ']', ' ');
  if (!ParseNumbers(p, &cam->params)) { *err = path + ": no <params>"; return false; }
  return true;
}

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
  if (out(diff[0], lg) || out(diff[1], lg) || out(diff[2], lg)) {
    std::fprintf(stderr, "E IMU bias(es) for gyroscope differ (%g, %g, %g ) more than expected (%g)%s\n", diff[0], diff[1], diff[2], lg,
                 reference_sense ? " [reference comparison sense: '<', see -imu_diff_sense]" : "");
    return true;
  }
  if (out(diff[3], la) || out(diff[4], la) || out(diff[5], la)) {
    std::fprintf(stderr, "E IMU bias(es) for accelrometer differ (%g, %g, %g ) more than expected (%g)%s\n", diff[3], diff[4], diff[5], la,
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

// -undistort_dir: every input image of every camera through the calibrated model into a pinhole camera of the same size (intrinsics from
// vc_undistort_fit_linear at -undistort_alpha), in batches of at most 64 images per call; dir/cameras.xml is the rig with every camera
// replaced by that pinhole camera, T_ck kept, written by the calibrator's own XML writer
static bool UndistortInputs(vic::ViCalibrator& cal, const std::vector<std::string>& cam_globs, const std::vector<vic::CameraAndPose>& input_cameras,
                            bool calibrate_imu, int device, const std::string& dir, double alpha, std::string* err) {
  struct stat st;
  if (mkdir(dir.c_str(), 0777) != 0 && !(stat(dir.c_str(), &st) == 0 && S_ISDIR(st.st_mode))) {      // (one level: parents must exist)
    *err = "cannot create the directory " + dir;
    return false;
  }
  vic::ViCalibrator rig(device);
  rig.SetCalibrateImu(calibrate_imu);                 // (the XML writer's axis convention follows it)
  const int kBatch = 64;
  for (size_t c = 0; c < cam_globs.size(); ++c) {
    vic::CameraAndPose cam = cal.GetCamera(c);
    cam.model = input_cameras[c].model; cam.width = input_cameras[c].width; cam.height = input_cameras[c].height;
    const int w = cam.width, h = cam.height;
    const vic::LinearCamera dst = vic::Undistorter::FitLinear(cam, w, h, alpha);
    vic::Undistorter und(cal, (int)c, dst);
    std::vector<std::string> files;
    if (!GlobSorted(cam_globs[c], &files)) { *err = "no images match " + cam_globs[c]; return false; }
    std::vector<unsigned char> in, out, px;
    for (size_t first = 0; first < files.size(); first += kBatch) {
      const size_t n = std::min((size_t)kBatch, files.size() - first), np = (size_t)w * h;
      in.resize(n * np); out.resize(n * np);
      for (size_t k = 0; k < n; ++k) {
        int iw = 0, ih = 0;
        if (!ReadPgm(files[first + k], &iw, &ih, &px, err)) return false;
        if (iw != w || ih != h) { *err = files[first + k] + ": image size differs from the camera's"; return false; }
        std::memcpy(in.data() + k * np, px.data(), np);
      }
      und.Images((int)n, in.data(), w, (long long)np, out.data(), w, (long long)np);
      for (size_t k = 0; k < n; ++k) {
        std::string name = files[first + k];
        const size_t slash = name.find_last_of('/');
        if (slash != std::string::npos) name = name.substr(slash + 1);
        const size_t dot = name.find_last_of('.');
        if (dot != std::string::npos && dot > 0) name = name.substr(0, dot);
        const std::string path = dir + "/cam" + std::to_string(c) + "_" + name + ".pgm";
        FILE* f = std::fopen(path.c_str(), "wb");
        if (!f) { *err = "cannot write " + path; return false; }
        std::fprintf(f, "P5\n%d %d\n255\n", w, h);
        std::fwrite(out.data() + k * np, 1, np, f);
        std::fclose(f);
      }
    }
    vic::CameraAndPose lin;
    lin.model = VC_MODEL_LINEAR; lin.params.assign(dst.fu_fv_u0_v0.begin(), dst.fu_fv_u0_v0.end()); lin.width = w; lin.height = h; lin.T_ck = cam.T_ck;
    rig.AddCamera(lin);
    std::fprintf(stderr, "I camera %zu: %zu images undistorted into %s (pinhole fu %.6g fv %.6g u0 %.6g v0 %.6g)\n", c, files.size(), dir.c_str(),
                 dst.fu_fv_u0_v0[0], dst.fu_fv_u0_v0[1], dst.fu_fv_u0_v0[2], dst.fu_fv_u0_v0[3]);
  }
  rig.WriteCameraModels(dir + "/cameras.xml");
  return true;
}

// -rectify_cams a,b: two different cameras of the n_cam channels
static bool ParseRectifyCams(const std::string& s, size_t n_cam, int* a, int* b) {
  char tail = 0;
  if (std::sscanf(s.c_str(), "%d,%d%c", a, b, &tail) != 2) return false;
  return *a >= 0 && *b >= 0 && *a != *b && (size_t)*a < n_cam && (size_t)*b < n_cam;
}
static bool WritePgm(const std::string& path, int w, int h, const unsigned char* px, std::string* err) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) { *err = "cannot write " + path; return false; }
  std::fprintf(f, "P5\n%d %d\n255\n", w, h);
  std::fwrite(px, 1, (size_t)w * h, f);
  std::fclose(f);
  return true;
}
static std::string BaseName(std::string name) {
  const size_t slash = name.find_last_of('/');
  if (slash != std::string::npos) name = name.substr(slash + 1);
  const size_t dot = name.find_last_of('.');
  if (dot != std::string::npos && dot > 0) name = name.substr(0, dot);
  return name;
}

// -rectify_dir: cameras a and b of the result rectified (vc_rectifier: the rotations of vc_stereo_rectify_rotations, one pinhole camera of
// a's size for both from vc_stereo_fit_linear at -rectify_alpha).  dir/cameras.xml holds the two rectified cameras (T_ck_rect: they differ by
// a translation along x), dir/stereo_check.csv the stereo consistency check over the corners both cameras detected in the frames the
// calibration used, and with image input the i-th sorted image of a and of b are rectified as a pair, in batches of at most 64.
static bool RectifyOutputs(vic::ViCalibrator& cal, const std::vector<Channel>& channels, const std::vector<long>& frame_ids, int grid_n,
                           const std::vector<std::string>& cam_globs, bool from_images, const std::vector<vic::CameraAndPose>& input_cameras, bool calibrate_imu,
                           int device, const std::string& dir, int a, int b, double alpha, std::string* err) {
  struct stat st;
  if (mkdir(dir.c_str(), 0777) != 0 && !(stat(dir.c_str(), &st) == 0 && S_ISDIR(st.st_mode))) {      // (one level: parents must exist)
    *err = "cannot create the directory " + dir;
    return false;
  }
  const int cams[2] = {a, b};
  vic::LinearCamera dst;                                 // intrinsics left zero: fitted at alpha
  dst.width = input_cameras[a].width; dst.height = input_cameras[a].height;
  vic::Rectifier rect(cal, a, b, dst, alpha);
  dst = rect.Linear();
  const double baseline = rect.Baseline();
  // ---- cameras.xml
  {
    vic::ViCalibrator rig(device);
    rig.SetCalibrateImu(calibrate_imu);                  // (the XML writer's axis convention follows it)
    vic::Se3 T[2];
    rect.RectifiedPoses(&T[0], &T[1]);
    for (int s = 0; s < 2; ++s) {
      vic::CameraAndPose lin;
      lin.model = VC_MODEL_LINEAR; lin.params.assign(dst.fu_fv_u0_v0.begin(), dst.fu_fv_u0_v0.end()); lin.width = dst.width; lin.height = dst.height; lin.T_ck = T[s];
      rig.AddCamera(lin);
    }
    rig.WriteCameraModels(dir + "/cameras.xml");
  }
  // ---- stereo_check.csv: the two cameras' detections of the calibration's frames in the layout of vc_add_observation_tiles, matched by vc_match_tiles
  std::map<long, int> frame_index;
  for (size_t k = 0; k < frame_ids.size(); ++k) frame_index[frame_ids[k]] = (int)k;
  std::vector<int> tile_frame, tile_cam, point_id;
  std::vector<long long> tile_off(1, 0);
  std::vector<const Detection*> dets;
  for (int s = 0; s < 2; ++s) {
    std::map<int, std::vector<const Detection*>> per_frame;
    for (const Detection& d : channels[(size_t)cams[s]].det) {
      auto it = frame_index.find(d.frame);
      if (it == frame_index.end() || d.dot >= grid_n) continue;
      per_frame[it->second].push_back(&d);
    }
    for (const auto& kv : per_frame) {
      for (const Detection* d : kv.second) { point_id.push_back(d->dot); dets.push_back(d); }
      tile_frame.push_back(kv.first); tile_cam.push_back(s); tile_off.push_back((long long)dets.size());
    }
  }
  const vic::TileMatches m = vic::Rectifier::MatchTiles((int)tile_frame.size(), tile_frame.data(), tile_cam.data(), tile_off.data(), point_id.data(), 0, 1);
  const size_t n = m.pos_a.size(), nf = m.frame.size();
  std::vector<double> px_a(2 * n + 2), px_b(2 * n + 2), target(3 * n + 3);
  for (size_t k = 0; k < n; ++k) {
    const Detection* da = dets[(size_t)m.pos_a[k]]; const Detection* db = dets[(size_t)m.pos_b[k]];
    px_a[2 * k] = da->u; px_a[2 * k + 1] = da->v; px_b[2 * k] = db->u; px_b[2 * k + 1] = db->v;
    target[3 * k] = da->X; target[3 * k + 1] = da->Y; target[3 * k + 2] = da->Z;
  }
  const vic::StereoCheck chk = rect.Check(m.frame_off, px_a.data(), px_b.data(), target.data());
  FILE* f = std::fopen((dir + "/stereo_check.csv").c_str(), "w");
  if (!f) { *err = "cannot write " + dir + "/stereo_check.csv"; return false; }
  std::fprintf(f, "frame,pairs,invalid,mean_dv,rms_dv,max_abs_dv,mean_z_m,rigid_rms_m\n");
  double sum2 = 0.0, worst = 0.0; long long valid = 0;
  std::vector<double> rms;
  for (size_t k = 0; k < nf; ++k) {
    const int cnt = chk.count[k];
    std::fprintf(f, "%ld,%d,%d,%.10g,%.10g,%.10g,%.10g,%.10g\n", frame_ids[(size_t)m.frame[k]], cnt + chk.n_invalid[k], chk.n_invalid[k], cnt > 0 ? chk.sum_dv[k] / cnt : 0.0,
                 cnt > 0 ? std::sqrt(chk.sum_dv2[k] / cnt) : 0.0, chk.max_abs_dv[k], chk.mean_z[k], chk.rigid_rms[k]);
    sum2 += chk.sum_dv2[k]; valid += cnt; worst = std::max(worst, chk.max_abs_dv[k]);
    if (chk.rigid_rms[k] == chk.rigid_rms[k]) rms.push_back(chk.rigid_rms[k]);
  }
  std::fclose(f);
  std::sort(rms.begin(), rms.end());
  std::fprintf(stderr, "I cameras %d,%d rectified into %s: baseline %.6g m, %zu frames with %lld matched corners, rms dv %.4g px, worst |dv| %.4g px, median rigid_rms_m %.4g\n",
               a, b, dir.c_str(), baseline, nf, valid, valid > 0 ? std::sqrt(sum2 / (double)valid) : 0.0, worst, rms.empty() ? 0.0 : rms[rms.size() / 2]);
  if (!from_images) return true;
  // ---- the rectified images
  std::vector<std::string> files[2];
  for (int s = 0; s < 2; ++s)
    if (!GlobSorted(cam_globs[(size_t)cams[s]], &files[s])) { *err = "no images match " + cam_globs[(size_t)cams[s]]; return false; }
  const size_t n_img = std::min(files[0].size(), files[1].size());
  if (files[0].size() != files[1].size()) std::fprintf(stderr, "W cameras %d and %d have %zu and %zu images: the first %zu are rectified as pairs\n", a, b, files[0].size(), files[1].size(), n_img);
  const int kBatch = 64;
  const int sw[2] = {input_cameras[a].width, input_cameras[b].width}, sh[2] = {input_cameras[a].height, input_cameras[b].height};
  const size_t snp[2] = {(size_t)sw[0] * sh[0], (size_t)sw[1] * sh[1]}, dnp = (size_t)dst.width * dst.height;
  std::vector<unsigned char> in[2], out[2], px;
  for (size_t first = 0; first < n_img; first += kBatch) {
    const size_t nb = std::min((size_t)kBatch, n_img - first);
    for (int s = 0; s < 2; ++s) {
      in[s].resize(nb * snp[s]); out[s].resize(nb * dnp);
      for (size_t k = 0; k < nb; ++k) {
        int iw = 0, ih = 0;
        if (!ReadPgm(files[s][first + k], &iw, &ih, &px, err)) return false;
        if (iw != sw[s] || ih != sh[s]) { *err = files[s][first + k] + ": image size differs from the camera's"; return false; }
        std::memcpy(in[s].data() + k * snp[s], px.data(), snp[s]);
      }
    }
    rect.Pairs((int)nb, in[0].data(), sw[0], (long long)snp[0], in[1].data(), sw[1], (long long)snp[1], out[0].data(), dst.width, (long long)dnp, out[1].data(), dst.width,
               (long long)dnp);
    for (int s = 0; s < 2; ++s)
      for (size_t k = 0; k < nb; ++k)
        if (!WritePgm(dir + "/cam" + std::to_string(cams[s]) + "_" + BaseName(files[s][first + k]) + ".pgm", dst.width, dst.height, out[s].data() + k * dnp, err)) return false;
  }
  std::fprintf(stderr, "I %zu image pairs rectified into %s (pinhole fu %.6g fv %.6g u0 %.6g v0 %.6g)\n", n_img, dir.c_str(), dst.fu_fv_u0_v0[0], dst.fu_fv_u0_v0[1],
               dst.fu_fv_u0_v0[2], dst.fu_fv_u0_v0[3]);
  return true;
}

// ---- -compare_models / -compare_to: two calibrations compared in pixel space (vc_compar*) ---------------------------------------------
// every <camera> of a calibu rig XML with its pose: the inverse of vc_write_camera_models.  T_wc = [M | t] with M = R_ck^T RDF^T and
// t = -R_ck^T t_ck, RDF the matrix of the <right>, <down> and <forward> rows (the identity when they are missing).
static bool ReadRigFile(const std::string& path, std::vector<vic::CameraAndPose>* cams, std::string* err) {
  std::ifstream f(path);
  if (!f) { *err = "cannot open rig file " + path; return false; }
  std::stringstream ss; ss << f.rdbuf();
  const std::string s = ss.str();
  cams->clear();
  auto numbers = [](std::string t, std::vector<double>* v) {
    for (char& ch : t) if (ch == '[' || ch == ']') ch = ' ';
    return ParseNumbers(t, v);
  };
  for (size_t from = 0;;) {
    const size_t p = s.find("<camera>", from);
    if (p == std::string::npos) break;
    const size_t q = s.find("</camera>", p);
    if (q == std::string::npos) { *err = path + ": <camera> without </camera>"; return false; }
    const std::string c = s.substr(p, q - p);
    from = q + 9;
    const std::string where = path + ": camera " + std::to_string(cams->size());
    vic::CameraAndPose cam;
    const std::string head = Between(c, "<camera_model", ">");
    cam.model = ModelId(Between(head, "type=\"", "\""));
    if (cam.model < 0) { *err = where + ": unsupported camera model type '" + Between(head, "type=\"", "\"") + "'"; return false; }
    std::vector<double> v;
    if (!numbers(Between(c, "<width>", "</width>"), &v) || v.size() != 1 || !(v[0] >= 2 && v[0] <= 8192)) { *err = where + ": no usable <width>"; return false; }
    cam.width = (int)v[0];
    if (!numbers(Between(c, "<height>", "</height>"), &v) || v.size() != 1 || !(v[0] >= 2 && v[0] <= 8192)) { *err = where + ": no usable <height>"; return false; }
    cam.height = (int)v[0];
    static const int kParams[6] = {5, 6, 7, 8, 4, 10};
    if (!numbers(Between(c, "<params>", "</params>"), &cam.params) || (int)cam.params.size() != kParams[cam.model]) {
      *err = where + ": <params> does not hold the " + std::to_string(kParams[cam.model]) + " parameters of " + ModelName(cam.model); return false;
    }
    double rdf[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const char* rows[3] = {"right", "down", "forward"};
    for (int r = 0; r < 3; ++r) {
      const std::string t = Between(c, std::string("<") + rows[r] + ">", std::string("</") + rows[r] + ">");
      if (t.empty()) continue;
      if (!numbers(t, &v) || v.size() != 3) { *err = where + ": <" + rows[r] + "> does not hold 3 numbers"; return false; }
      for (int k = 0; k < 3; ++k) rdf[3 * r + k] = v[k];
    }
    if (!numbers(Between(c, "<T_wc>", "</T_wc>"), &v) || v.size() != 12) { *err = where + ": <T_wc> does not hold 3 x 4 numbers"; return false; }
    // R_ck^T = M RDF; R_ck = its transpose; t_ck = -R_ck t
    double Rt[9], R[9];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Rt[3 * i + j] = v[4 * i] * rdf[j] + v[4 * i + 1] * rdf[3 + j] + v[4 * i + 2] * rdf[6 + j];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R[3 * i + j] = Rt[3 * j + i];
    double ortho = 0.0;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j)
      ortho = std::max(ortho, std::fabs(R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2] - (i == j ? 1.0 : 0.0)));
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    if (!(ortho <= 1e-6) || !(det > 0.0)) { *err = where + ": <T_wc> and the axis rows do not give a rotation"; return false; }
    double* T = cam.T_ck.data();
    // Shepperd: the unit quaternion [x y z w] of R_ck
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0.0) { const double k = 2.0 * std::sqrt(tr + 1.0); T[3] = 0.25 * k; T[0] = (R[7] - R[5]) / k; T[1] = (R[2] - R[6]) / k; T[2] = (R[3] - R[1]) / k; }
    else if (R[0] > R[4] && R[0] > R[8]) { const double k = 2.0 * std::sqrt(1.0 + R[0] - R[4] - R[8]); T[3] = (R[7] - R[5]) / k; T[0] = 0.25 * k; T[1] = (R[1] + R[3]) / k; T[2] = (R[2] + R[6]) / k; }
    else if (R[4] > R[8]) { const double k = 2.0 * std::sqrt(1.0 + R[4] - R[0] - R[8]); T[3] = (R[2] - R[6]) / k; T[0] = (R[1] + R[3]) / k; T[1] = 0.25 * k; T[2] = (R[5] + R[7]) / k; }
    else { const double k = 2.0 * std::sqrt(1.0 + R[8] - R[0] - R[4]); T[3] = (R[3] - R[1]) / k; T[0] = (R[2] + R[6]) / k; T[1] = (R[5] + R[7]) / k; T[2] = 0.25 * k; }
    const double qn = std::sqrt(T[0] * T[0] + T[1] * T[1] + T[2] * T[2] + T[3] * T[3]);
    for (int k = 0; k < 4; ++k) T[k] /= qn;
    for (int i = 0; i < 3; ++i) T[4 + i] = -(R[3 * i] * v[3] + R[3 * i + 1] * v[7] + R[3 * i + 2] * v[11]);
    cams->push_back(cam);
  }
  if (cams->empty()) { *err = path + ": no <camera>"; return false; }
  return true;
}
// -compare_grid GXxGY
static bool ParseCompareGrid(const std::string& s, int* gx, int* gy) {
  int a = 0, b = 0; char tail = 0;
  if (std::sscanf(s.c_str(), "%dx%d%c", &a, &b, &tail) != 2 || a < 2 || b < 2 || (long long)a * b > (1LL << 22)) return false;
  *gx = a; *gy = b;
  return true;
}
struct CompareOptions { std::string dir; int gx = 64, gy = 48, rings = 8; double fit_radius = 0.5; bool identity = false; };      // identity: no implied rotation is fitted
// the flags of a comparison, checked before anything else runs
static bool CompareFlags(CompareOptions* o, std::string* err) {
  o->dir = FlagString("compare_dir");
  if (o->dir.empty()) { *err = "-compare_models / -compare_to need -compare_dir"; return false; }
  if (!ParseCompareGrid(FlagString("compare_grid"), &o->gx, &o->gy)) { *err = "illegal value '" + FlagString("compare_grid") + "' specified for flag 'compare_grid': expected GXxGY, both at least 2, at most 2^22 samples"; return false; }
  o->fit_radius = FlagDouble("compare_fit_radius");
  if (!(o->fit_radius > 0.0 && o->fit_radius <= 1e6)) { *err = "illegal value for flag 'compare_fit_radius': expected a radius above 0"; return false; }
  o->rings = (int)FlagInt("compare_rings");
  if (o->rings < 1 || o->rings > 64) { *err = "illegal value for flag 'compare_rings': expected 1 ... 64"; return false; }
  return true;
}
// what can be said about two rigs before a device is looked for
static bool ComparableRigs(const std::vector<vic::CameraAndPose>& A, const std::vector<vic::CameraAndPose>& B, const CompareOptions& o, std::string* err) {
  if (A.size() != B.size()) { *err = "the two calibrations have " + std::to_string(A.size()) + " and " + std::to_string(B.size()) + " cameras"; return false; }
  for (size_t c = 0; c < A.size(); ++c) {
    if (A[c].width != B[c].width || A[c].height != B[c].height) {
      *err = "camera " + std::to_string(c) + ": image sizes " + std::to_string(A[c].width) + "x" + std::to_string(A[c].height) + " and " + std::to_string(B[c].width) + "x" +
             std::to_string(B[c].height) + " differ";
      return false;
    }
    if (o.gx > A[c].width || o.gy > A[c].height) { *err = "camera " + std::to_string(c) + ": -compare_grid exceeds the image"; return false; }
  }
  return true;
}
// Compares A with B camera by camera and writes the files of -compare_dir.  Exit status: 0, 1 (an error, said in *err) or 3 (no device).
static int CompareRigs(const std::vector<vic::CameraAndPose>& A, const std::vector<vic::CameraAndPose>& B, const CompareOptions& o, int device, std::string* err) {
  if (!ComparableRigs(A, B, o, err)) return 1;
  struct stat st;
  if (mkdir(o.dir.c_str(), 0777) != 0 && !(stat(o.dir.c_str(), &st) == 0 && S_ISDIR(st.st_mode))) { *err = "cannot create the directory " + o.dir; return 1; }      // (one level)
  FILE* fs = std::fopen((o.dir + "/compare_summary.csv").c_str(), "w");
  if (!fs) { *err = "cannot write into " + o.dir; return 1; }
  std::fprintf(fs, "camera,model_a,model_b,rx_deg,ry_deg,rz_deg,status,iterations,n_fit,count,invalid,rms_px,max_px,count_plain,rms_plain_px,max_plain_px\n");
  std::vector<vic::CompareRings> rings(A.size());
  std::vector<std::array<double, 9>> implied(A.size());
  int rc = 0;
  for (size_t c = 0; c < A.size() && rc == 0; ++c) {
    vc_comparer* h = nullptr;
    const int st_create = vc_comparer_create(device, A[c].model, A[c].params.data(), (int)A[c].params.size(), B[c].model, B[c].params.data(), (int)B[c].params.size(),
                                             A[c].width, A[c].height, o.gx, o.gy, &h);
    if (st_create == VC_ERR_NO_DEVICE) { *err = "no HIP device (there is no CPU fallback)"; rc = 3; break; }
    if (st_create != VC_OK) { *err = "camera " + std::to_string(c) + ": the comparison refuses these cameras (status " + std::to_string(st_create) + ")"; rc = 1; break; }
    const size_t n = (size_t)o.gx * o.gy;
    std::vector<double> d(2 * n);
    std::vector<unsigned char> fl(n);
    vic::CompareFit fit;
    vic::CompareSummary s, sp;
    int q = vc_compare_run(h, o.identity ? 0.0 : o.fit_radius, 0, nullptr);
    if (q == VC_OK) q = vc_compare_get_fit(h, fit.R_ba, &fit.status, &fit.iterations, &fit.n_fit, &fit.n_left_out, &fit.cost0, &fit.cost);
    if (q == VC_OK) q = vc_compare_get_map(h, d.data(), fl.data());
    if (q == VC_OK) q = vc_compare_summary(h, &s.count, &s.invalid, &s.sum_du, &s.sum_dv, &s.sum_sq, &s.max_err, &s.worst);
    vic::CompareRings& r = rings[c];
    r.count.resize(o.rings); r.invalid.resize(o.rings); r.sum_sq.resize(o.rings); r.max_err.resize(o.rings);
    if (q == VC_OK) q = vc_compare_rings(h, o.rings, r.count.data(), r.invalid.data(), r.sum_sq.data(), r.max_err.data());
    if (q == VC_OK) q = vc_compare_run(h, 0.0, 0, nullptr);                                  // ... and at R = I
    if (q == VC_OK) q = vc_compare_summary(h, &sp.count, &sp.invalid, &sp.sum_du, &sp.sum_dv, &sp.sum_sq, &sp.max_err, &sp.worst);
    vc_comparer_destroy(h);
    if (q != VC_OK) {
      *err = "camera " + std::to_string(c) + (q == VC_ERR_NUMERIC ? ": the implied rotation cannot be fitted (fewer than 3 samples within -compare_fit_radius that both calibrations have an image of, or a degenerate system)"
                                                                  : ": the comparison failed (status " + std::to_string(q) + ")");
      rc = q == VC_ERR_NO_DEVICE ? 3 : 1; break;
    }
    std::memcpy(implied[c].data(), fit.R_ba, 72);
    FILE* fm = std::fopen((o.dir + "/compare_cam" + std::to_string(c) + ".csv").c_str(), "w");
    if (!fm) { *err = "cannot write into " + o.dir; rc = 1; break; }
    std::fprintf(fm, "x,y,du,dv,flags\n");
    for (size_t k = 0; k < n; ++k) {
      const int i = (int)(k % o.gx), j = (int)(k / o.gx);
      std::fprintf(fm, "%.17g,%.17g,%.17g,%.17g,%d\n", (double)(i * (A[c].width - 1)) / (o.gx - 1), (double)(j * (A[c].height - 1)) / (o.gy - 1), d[2 * k], d[2 * k + 1], (int)fl[k]);
    }
    std::fclose(fm);
    // the implied rotation as a rotation vector
    const double* R = fit.R_ba;
    const double vx = 0.5 * (R[7] - R[5]), vy = 0.5 * (R[2] - R[6]), vz = 0.5 * (R[3] - R[1]), sn = std::sqrt(vx * vx + vy * vy + vz * vz);
    const double ang = std::atan2(sn, 0.5 * (R[0] + R[4] + R[8] - 1.0)), k = sn > 0.0 ? ang / sn * 180.0 / M_PI : 0.0;
    std::fprintf(fs, "%zu,%s,%s,%.17g,%.17g,%.17g,%d,%d,%d,%lld,%lld,%.17g,%.17g,%lld,%.17g,%.17g\n", c, ModelName(A[c].model), ModelName(B[c].model), k * vx, k * vy, k * vz,
                 fit.status, fit.iterations, fit.n_fit, s.count, s.invalid, s.count > 0 ? std::sqrt(s.sum_sq / s.count) : 0.0, s.max_err, sp.count,
                 sp.count > 0 ? std::sqrt(sp.sum_sq / sp.count) : 0.0, sp.max_err);
    std::fprintf(stderr, "I camera %zu (%s against %s): implied rotation %.4g deg, %.4g px rms (%.4g px max) over %lld samples; %.4g px rms without it\n", c,
                 ModelName(A[c].model), ModelName(B[c].model), ang * 180.0 / M_PI, s.count > 0 ? std::sqrt(s.sum_sq / s.count) : 0.0, s.max_err, s.count,
                 sp.count > 0 ? std::sqrt(sp.sum_sq / sp.count) : 0.0);
  }
  if (rc == 0) {                                         // the second table of the summary: one row per camera and ring, at the implied rotation
    std::fprintf(fs, "camera,ring,rho_from,rho_to,count,invalid,rms_px,max_px\n");
    for (size_t c = 0; c < A.size(); ++c)
      for (int k = 0; k < o.rings; ++k)
        std::fprintf(fs, "%zu,%d,%.17g,%.17g,%lld,%lld,%.17g,%.17g\n", c, k, (double)k / o.rings, (double)(k + 1) / o.rings, rings[c].count[k], rings[c].invalid[k],
                     rings[c].count[k] > 0 ? std::sqrt(rings[c].sum_sq[k] / rings[c].count[k]) : 0.0, rings[c].max_err[k]);
  }
  std::fclose(fs);
  if (rc == 0 && A.size() > 1) {
    FILE* fe = std::fopen((o.dir + "/compare_extrinsics.csv").c_str(), "w");
    if (!fe) { *err = "cannot write into " + o.dir; return 1; }
    std::fprintf(fe, "camera,angle_deg,distance_m,angle_plain_deg,distance_plain_m,a_qx,a_qy,a_qz,a_qw,a_tx,a_ty,a_tz,b_qx,b_qy,b_qz,b_qw,b_tx,b_ty,b_tz\n");
    for (size_t c = 0; c < A.size(); ++c) {              // (camera 0 against itself: a row of zeros that carries its two poses)
      double out[4];
      if (vc_compare_extrinsics(A[0].T_ck.data(), A[c].T_ck.data(), B[0].T_ck.data(), B[c].T_ck.data(), implied[0].data(), implied[c].data(), out) != VC_OK) {
        *err = "camera " + std::to_string(c) + ": the poses cannot be compared"; std::fclose(fe); return 1;
      }
      std::fprintf(fe, "%zu,%.17g,%.17g,%.17g,%.17g", c, out[0] * 180.0 / M_PI, out[1], out[2] * 180.0 / M_PI, out[3]);
      for (const vic::CameraAndPose* cam : {&A[c], &B[c]}) for (int k = 0; k < 7; ++k) std::fprintf(fe, ",%.17g", cam->T_ck.v[k]);
      std::fprintf(fe, "\n");
    }
    std::fclose(fe);
  }
  return rc;
}

// ---- -register_*: a depth image of camera s registered into camera d, and d's image into s (vc_regist*) ----------------------------------
// 16-bit binary PGM, maxval 65535, most significant byte first (the Netpbm rule)
static bool ReadPgm16(const std::string& path, int* w, int* h, std::vector<unsigned short>* px, std::string* err) {
  std::ifstream f(path, std::ios::binary);
  if (!f) { *err = "cannot open image " + path; return false; }
  std::string magic; f >> magic;
  if (magic != "P5") { *err = path + ": not a binary PGM (P5)"; return false; }
  auto next_int = [&](long* v) {
    while (true) { f >> std::ws; if (f.peek() == '#') { std::string c; std::getline(f, c); } else break; }
    return (bool)(f >> *v);
  };
  long W = 0, H = 0, M = 0;
  if (!next_int(&W) || !next_int(&H) || !next_int(&M) || W < 1 || H < 1 || M != 65535) { *err = path + ": expected a 16-bit PGM header (maxval 65535)"; return false; }
  if (W > 8192 || H > 8192) { *err = path + ": " + std::to_string(W) + " x " + std::to_string(H) + " pixels, more than the 8192 x 8192 a camera can have"; return false; }
  f.get();                                          // the single whitespace byte behind the header
  std::vector<unsigned char> raw((size_t)W * H * 2);
  f.read((char*)raw.data(), (std::streamsize)raw.size());
  if ((size_t)f.gcount() != raw.size()) { *err = path + ": truncated image data"; return false; }
  px->resize((size_t)W * H);
  for (size_t k = 0; k < px->size(); ++k) (*px)[k] = (unsigned short)((raw[2 * k] << 8) | raw[2 * k + 1]);
  *w = (int)W; *h = (int)H;
  return true;
}
static bool WritePgm16(const std::string& path, int w, int h, const unsigned short* px, std::string* err) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) { *err = "cannot write " + path; return false; }
  std::fprintf(f, "P5\n%d %d\n65535\n", w, h);
  std::vector<unsigned char> raw((size_t)w * h * 2);
  for (size_t k = 0; k < (size_t)w * h; ++k) { raw[2 * k] = (unsigned char)(px[k] >> 8); raw[2 * k + 1] = (unsigned char)(px[k] & 255); }
  const bool written = std::fwrite(raw.data(), 1, raw.size(), f) == raw.size();
  if (std::fclose(f) != 0 || !written) { *err = "cannot write " + path + " in full"; return false; }
  return true;
}
struct RegisterOptions { bool on = false; int s = 0, d = 1, kind = 0, splat = 0; double unit = 0.001, occl_tol = 10.0; std::string depth, color, dir; };
// the flags of a registration, checked before anything else runs
static bool RegisterFlags(RegisterOptions* o, std::string* err) {
  o->depth = FlagString("register_depth"); o->color = FlagString("register_color"); o->dir = FlagString("register_dir");
  o->on = !o->depth.empty() || !FlagString("register_models").empty();
  if (!o->on) return true;
  if (o->depth.empty() || o->dir.empty()) { *err = "-register_models / -register_depth need -register_depth and -register_dir"; return false; }
  char tail = 0;
  if (std::sscanf(FlagString("register_cams").c_str(), "%d,%d%c", &o->s, &o->d, &tail) != 2 || o->s < 0 || o->d < 0) {
    *err = "illegal value '" + FlagString("register_cams") + "' specified for flag 'register_cams': expected s,d"; return false;
  }
  o->unit = FlagDouble("register_unit");
  if (!(o->unit > 0.0 && o->unit <= 1e6)) { *err = "illegal value for flag 'register_unit': expected metres per count above 0"; return false; }
  const std::string kind = FlagString("register_kind"), splat = FlagString("register_splat");
  if (kind != "z" && kind != "range") { *err = "illegal value '" + kind + "' specified for flag 'register_kind': expected z or range"; return false; }
  if (splat != "nearest" && splat != "footprint") { *err = "illegal value '" + splat + "' specified for flag 'register_splat': expected nearest or footprint"; return false; }
  o->kind = kind == "range" ? 1 : 0; o->splat = splat == "footprint" ? 1 : 0;
  o->occl_tol = FlagDouble("register_occlusion_tol");
  if (!(o->occl_tol >= 0.0 && o->occl_tol <= 1e300)) { *err = "illegal value for flag 'register_occlusion_tol': expected a tolerance of at least 0"; return false; }
  return true;
}
// Registers the depth images of camera s into camera d, in batches of at most 16.  Everything that can be said without a device -- camera
// indices, file counts, image sizes -- is said first.  Exit status: 0, 1 (an error said in *err) or 3 (no device).
static int RegisterRig(const std::vector<vic::CameraAndPose>& cams, const RegisterOptions& o, int device, std::string* err) {
  if ((size_t)o.s >= cams.size() || (size_t)o.d >= cams.size()) {
    *err = "illegal value for flag 'register_cams': camera " + std::to_string(std::max(o.s, o.d)) + " of a rig of " + std::to_string(cams.size()) + " cameras"; return 1;
  }
  const vic::CameraAndPose& S = cams[o.s];
  const vic::CameraAndPose& D = cams[o.d];
  std::vector<std::string> dfiles, cfiles;
  if (!GlobSorted(StripScheme(o.depth), &dfiles)) { *err = "no depth image matches " + o.depth; return 1; }
  if (!o.color.empty()) {
    if (!GlobSorted(StripScheme(o.color), &cfiles)) { *err = "no image matches " + o.color; return 1; }
    if (cfiles.size() != dfiles.size()) { *err = "-register_depth matches " + std::to_string(dfiles.size()) + " files and -register_color " + std::to_string(cfiles.size()); return 1; }
  }
  const size_t ns = (size_t)S.width * S.height, nd = (size_t)D.width * D.height, n = dfiles.size();
  std::vector<unsigned short> depth(ns * n);
  std::vector<unsigned char> color(cfiles.empty() ? 0 : nd * n);
  for (size_t k = 0; k < n; ++k) {
    int w = 0, h = 0;
    std::vector<unsigned short> px;
    if (!ReadPgm16(dfiles[k], &w, &h, &px, err)) return 1;
    if (w != S.width || h != S.height) { *err = dfiles[k] + ": " + std::to_string(w) + " x " + std::to_string(h) + " pixels, camera " + std::to_string(o.s) + " has " + std::to_string(S.width) + " x " + std::to_string(S.height); return 1; }
    std::copy(px.begin(), px.end(), depth.begin() + k * ns);
    if (cfiles.empty()) continue;
    std::vector<unsigned char> c8;
    if (!ReadPgm(cfiles[k], &w, &h, &c8, err)) return 1;
    if (w != D.width || h != D.height) { *err = cfiles[k] + ": " + std::to_string(w) + " x " + std::to_string(h) + " pixels, camera " + std::to_string(o.d) + " has " + std::to_string(D.width) + " x " + std::to_string(D.height); return 1; }
    std::copy(c8.begin(), c8.end(), color.begin() + k * nd);
  }
  struct stat st;
  if (mkdir(o.dir.c_str(), 0777) != 0 && !(stat(o.dir.c_str(), &st) == 0 && S_ISDIR(st.st_mode))) { *err = "cannot create the directory " + o.dir; return 1; }      // (one level)
  vc_registrar* r = nullptr;
  const int st_create = vc_registrar_create(device, S.model, S.params.data(), (int)S.params.size(), S.width, S.height, S.T_ck.data(), D.model, D.params.data(),
                                            (int)D.params.size(), D.width, D.height, D.T_ck.data(), o.unit, o.unit, o.kind, o.splat, &r);
  if (st_create == VC_ERR_NO_DEVICE) { *err = "no HIP device (there is no CPU fallback)"; return 3; }
  if (st_create != VC_OK) { *err = "the registration refuses these cameras (status " + std::to_string(st_create) + ")"; return 1; }
  FILE* csv = std::fopen((o.dir + "/register_summary.csv").c_str(), "w");
  if (!csv) { vc_registrar_destroy(r); *err = "cannot write " + o.dir + "/register_summary.csv"; return 1; }
  std::fprintf(csv, "image,zero,no_ray,behind,outside,value_range,footprint,candidates,filled\n");
  long long filled = 0, candidates = 0;
  int status = 0;
  for (size_t first = 0; first < n && status == 0; first += 16) {
    const int m = (int)std::min<size_t>(16, n - first);
    std::vector<unsigned short> out(nd * m);
    std::vector<long long> cnt(8 * (size_t)m);
    int q = vc_register_depth(r, m, depth.data() + first * ns, 2 * S.width, (long long)(2 * ns), out.data(), 2 * D.width, (long long)(2 * nd), nullptr, cnt.data());
    std::vector<unsigned char> cin;
    if (q == VC_OK && !cfiles.empty()) {
      cin.resize(ns * m);
      q = vc_register_color(r, m, depth.data() + first * ns, 2 * S.width, (long long)(2 * ns), color.data() + first * nd, D.width, (long long)nd, o.occl_tol, 0, cin.data(),
                            S.width, (long long)ns, nullptr);
    }
    if (q != VC_OK) { *err = "the registration failed (status " + std::to_string(q) + ")"; status = q == VC_ERR_NO_DEVICE ? 3 : 1; break; }
    for (int k = 0; k < m && status == 0; ++k) {
      const std::string name = BaseName(dfiles[first + k]);
      if (!WritePgm16(o.dir + "/" + name + ".pgm", D.width, D.height, out.data() + k * nd, err)) status = 1;
      if (status == 0 && !cfiles.empty() && !WritePgm(o.dir + "/color_in_depth_" + name + ".pgm", S.width, S.height, cin.data() + k * ns, err)) status = 1;
      std::fprintf(csv, "%s", name.c_str());
      for (int c = 0; c < 8; ++c) std::fprintf(csv, ",%lld", cnt[8 * (size_t)k + c]);
      std::fprintf(csv, "\n");
      candidates += cnt[8 * (size_t)k + 6]; filled += cnt[8 * (size_t)k + 7];
    }
  }
  if (std::fclose(csv) != 0 && status == 0) { *err = "cannot write " + o.dir + "/register_summary.csv in full"; status = 1; }
  vc_registrar_destroy(r);
  if (status != 0) return status;
  std::printf("registered %zu depth images of camera %d (%s) into camera %d (%s), %s: %lld candidates, %lld pixels filled -> %s\n", n, o.s, ModelName(S.model), o.d,
              ModelName(D.model), o.splat ? "footprint" : "nearest", candidates, filled, o.dir.c_str());
  return 0;
}

// ---- -depthcal_*: the range error of a depth camera against the target, and its correction (vc_depthcal*) ------------------------------
struct DepthCalCli {
  bool on = false, apply = false;
  int cam = 0, kind = 0, bx = 4, by = 3, degree = 2, min_count = 50, interp = 0;
  double unit = 0.001, v_ref = 1000.0, min_cos = 0.5, max_dev = 100.0, min_spread = 0.02, rect[4] = {0, 0, 0, 0};
  std::string models, poses, depth, dir, file;
};
// the flags of a depth calibration, checked before anything else runs
static bool DepthCalFlags(DepthCalCli* o, std::string* err) {
  o->models = FlagString("depthcal_models"); o->poses = FlagString("depthcal_poses"); o->depth = FlagString("depthcal_depth"); o->dir = FlagString("depthcal_dir");
  o->file = FlagString("depthcal_apply");
  o->apply = !o->file.empty();
  o->on = !o->models.empty() || !o->poses.empty() || !o->depth.empty() || o->apply;
  if (!o->on) return true;
  if (o->depth.empty() || o->dir.empty()) { *err = "-depthcal_models / -depthcal_depth / -depthcal_apply need -depthcal_depth and -depthcal_dir"; return false; }
  if (o->apply && (!o->models.empty() || !o->poses.empty())) { *err = "-depthcal_apply and -depthcal_models / -depthcal_poses exclude each other"; return false; }
  if (!o->apply && o->models.empty() != o->poses.empty()) { *err = "-depthcal_models and -depthcal_poses need each other"; return false; }
  o->cam = (int)FlagInt("depthcal_cam");
  if (o->cam < 0) { *err = "illegal value for flag 'depthcal_cam': expected a camera index"; return false; }
  o->unit = FlagDouble("depthcal_unit");
  if (!(o->unit > 0.0 && o->unit <= 1e6)) { *err = "illegal value for flag 'depthcal_unit': expected metres per count above 0"; return false; }
  const std::string kind = FlagString("depthcal_kind"), interp = FlagString("depthcal_interp");
  if (kind != "z" && kind != "range") { *err = "illegal value '" + kind + "' specified for flag 'depthcal_kind': expected z or range"; return false; }
  if (interp != "cell" && interp != "bilinear") { *err = "illegal value '" + interp + "' specified for flag 'depthcal_interp': expected cell or bilinear"; return false; }
  o->kind = kind == "range" ? 1 : 0; o->interp = interp == "bilinear" ? 1 : 0;
  char tail = 0;
  if (std::sscanf(FlagString("depthcal_bins").c_str(), "%d,%d%c", &o->bx, &o->by, &tail) != 2 || o->bx < 1 || o->by < 1 || o->bx > 32 || o->by > 32) {
    *err = "illegal value '" + FlagString("depthcal_bins") + "' specified for flag 'depthcal_bins': expected bx,by of 1..32 each"; return false;
  }
  o->v_ref = FlagDouble("depthcal_vref"); o->min_cos = FlagDouble("depthcal_min_cos"); o->max_dev = FlagDouble("depthcal_max_dev");
  o->degree = (int)FlagInt("depthcal_degree"); o->min_count = (int)FlagInt("depthcal_min_count"); o->min_spread = FlagDouble("depthcal_min_spread");
  if (!(o->v_ref > 0.0 && o->v_ref <= 1e300)) { *err = "illegal value for flag 'depthcal_vref': expected counts above 0"; return false; }
  if (!(o->min_cos > 0.0 && o->min_cos <= 1.0)) { *err = "illegal value for flag 'depthcal_min_cos': expected a cosine in (0, 1]"; return false; }
  if (!(o->max_dev > 0.0 && o->max_dev <= 1e300)) { *err = "illegal value for flag 'depthcal_max_dev': expected counts above 0"; return false; }
  if (o->degree < 0 || o->degree > 2) { *err = "illegal value for flag 'depthcal_degree': expected 0, 1 or 2"; return false; }
  if (o->min_count < 1) { *err = "illegal value for flag 'depthcal_min_count': expected at least 1"; return false; }
  if (!(o->min_spread >= 0.0 && o->min_spread <= 1e300)) { *err = "illegal value for flag 'depthcal_min_spread': expected at least 0"; return false; }
  const double margin = FlagDouble("depthcal_margin"), sp = FlagDouble("grid_spacing");
  const double gw = (double)(FlagInt("grid_width") - 1) * sp, gh = (double)(FlagInt("grid_height") - 1) * sp;
  o->rect[0] = -margin; o->rect[1] = -margin; o->rect[2] = gw + margin; o->rect[3] = gh + margin;
  if (!std::isfinite(margin) || !(o->rect[0] < o->rect[2] && o->rect[1] < o->rect[3])) { *err = "illegal value for flag 'depthcal_margin': the board rectangle is empty"; return false; }
  return true;
}
// a pose file in the format -save_poses writes: lines of 12 numbers, the top three rows of T_wk, '%' starts a comment -> [q (x y z w), t]
static bool ReadPoseFile(const std::string& path, std::vector<std::array<double, 7>>* poses, std::string* err) {
  std::ifstream f(path);
  if (!f) { *err = "cannot open pose file " + path; return false; }
  std::string line;
  while (std::getline(f, line)) {
    if (line.find_first_not_of(" \t\r") == std::string::npos || line[line.find_first_not_of(" \t\r")] == '%') continue;
    double m[12];
    std::istringstream is(line);
    for (int k = 0; k < 12; ++k) if (!(is >> m[k])) { *err = path + ": expected 12 numbers in a line"; return false; }
    const double R[9] = {m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]};
    double q[4];                                         // the largest of the four components first (Shepperd), then unit length
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0.0) { const double s = std::sqrt(tr + 1.0) * 2.0; q[3] = 0.25 * s; q[0] = (R[7] - R[5]) / s; q[1] = (R[2] - R[6]) / s; q[2] = (R[3] - R[1]) / s; }
    else if (R[0] > R[4] && R[0] > R[8]) { const double s = std::sqrt(1.0 + R[0] - R[4] - R[8]) * 2.0; q[3] = (R[7] - R[5]) / s; q[0] = 0.25 * s; q[1] = (R[1] + R[3]) / s; q[2] = (R[2] + R[6]) / s; }
    else if (R[4] > R[8]) { const double s = std::sqrt(1.0 + R[4] - R[0] - R[8]) * 2.0; q[3] = (R[2] - R[6]) / s; q[0] = (R[1] + R[3]) / s; q[1] = 0.25 * s; q[2] = (R[5] + R[7]) / s; }
    else { const double s = std::sqrt(1.0 + R[8] - R[0] - R[4]) * 2.0; q[3] = (R[3] - R[1]) / s; q[0] = (R[2] + R[6]) / s; q[1] = (R[5] + R[7]) / s; q[2] = 0.25 * s; }
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (!(n > 0.5 && n < 2.0)) { *err = path + ": a line holds no rotation"; return false; }
    poses->push_back({{q[0] / n, q[1] / n, q[2] / n, q[3] / n, m[3], m[7], m[11]}});
  }
  return true;
}
static bool ReadDepthFiles(const std::vector<std::string>& files, int w, int h, const std::string& who, std::vector<unsigned short>* depth, std::string* err) {
  const size_t ns = (size_t)w * h;
  for (size_t k = 0; k < files.size(); ++k) {
    int fw = 0, fh = 0;
    std::vector<unsigned short> px;
    if (!ReadPgm16(files[k], &fw, &fh, &px, err)) return false;
    if (k == 0 && w == 0) { w = fw; h = fh; }
    if (fw != w || fh != h) { *err = files[k] + ": " + std::to_string(fw) + " x " + std::to_string(fh) + " pixels, " + who + " has " + std::to_string(w) + " x " + std::to_string(h); return false; }
    depth->insert(depth->end(), px.begin(), px.end());
  }
  (void)ns;
  return true;
}
static bool MakeDir(const std::string& dir, std::string* err) {
  struct stat st;
  if (mkdir(dir.c_str(), 0777) != 0 && !(stat(dir.c_str(), &st) == 0 && S_ISDIR(st.st_mode))) { *err = "cannot create the directory " + dir; return false; }      // (one level)
  return true;
}
// Fits the correction of camera o.cam from the depth images and the frames' poses (n x 7), in batches of at most 16.  Everything that can be
// said without a device is said first.  Exit status: 0, 1 (an error said in *err) or 3 (no device).
static int DepthCalFit(const std::vector<vic::CameraAndPose>& cams, const std::vector<std::array<double, 7>>& poses, const char* poses_from, const DepthCalCli& o, int device,
                       std::string* err) {
  if ((size_t)o.cam >= cams.size()) { *err = "illegal value for flag 'depthcal_cam': camera " + std::to_string(o.cam) + " of a rig of " + std::to_string(cams.size()) + " cameras"; return 1; }
  const vic::CameraAndPose& S = cams[o.cam];
  std::vector<std::string> files;
  if (!GlobSorted(StripScheme(o.depth), &files)) { *err = "no depth image matches " + o.depth; return 1; }
  if (files.size() != poses.size()) { *err = "-depthcal_depth matches " + std::to_string(files.size()) + " files and " + poses_from + " has " + std::to_string(poses.size()) + " frames"; return 1; }
  std::vector<unsigned short> depth;
  if (!ReadDepthFiles(files, S.width, S.height, "camera " + std::to_string(o.cam), &depth, err)) return 1;
  if (!MakeDir(o.dir, err)) return 1;
  vc_depthcal* d = nullptr;
  const int st_create = vc_depthcal_create(device, S.model, S.params.data(), (int)S.params.size(), S.width, S.height, S.T_ck.data(), o.unit, o.kind, o.rect, o.bx, o.by,
                                           o.v_ref, o.min_cos, o.max_dev, &d);
  if (st_create == VC_ERR_NO_DEVICE) { *err = "no HIP device (there is no CPU fallback)"; return 3; }
  if (st_create != VC_OK) { *err = "the depth calibration refuses this camera (status " + std::to_string(st_create) + ")"; return 1; }
  const size_t ns = (size_t)S.width * S.height, n = files.size();
  const int cells = o.bx * o.by;
  int status = 0;
  FILE* ff = std::fopen((o.dir + "/depthcal_frames.csv").c_str(), "w");
  if (!ff) { vc_depthcal_destroy(d); *err = "cannot write " + o.dir + "/depthcal_frames.csv"; return 1; }
  std::fprintf(ff, "image,zero,no_ray,behind,outside,grazing,value_range,gate,used,qx,qy,qz,qw,tx,ty,tz\n");
  for (size_t first = 0; first < n && status == 0; first += 16) {
    const int m = (int)std::min<size_t>(16, n - first);
    std::vector<long long> cnt(8 * (size_t)m);
    const int q = vc_depthcal_add(d, m, depth.data() + first * ns, 2 * S.width, (long long)(2 * ns), poses[first].data(), cnt.data());
    if (q != VC_OK) { *err = q == VC_ERR_BAD_ARG ? "a frame's pose is not a rigid motion" : "the accumulation failed (status " + std::to_string(q) + ")"; status = q == VC_ERR_NO_DEVICE ? 3 : 1; break; }
    for (int k = 0; k < m; ++k) {
      std::fprintf(ff, "%s", BaseName(files[first + k]).c_str());
      for (int c = 0; c < 8; ++c) std::fprintf(ff, ",%lld", cnt[8 * (size_t)k + c]);
      for (int c = 0; c < 7; ++c) std::fprintf(ff, ",%.17g", poses[first + k][c]);
      std::fprintf(ff, "\n");
    }
  }
  if (std::fclose(ff) != 0 && status == 0) { *err = "cannot write " + o.dir + "/depthcal_frames.csv in full"; status = 1; }
  std::vector<double> sums((size_t)cells * 9), a(cells), b(cells);
  std::vector<int> st(cells);
  double c[3], rms[3];
  long long total[8];
  if (status == 0) {
    int q = vc_depthcal_sums(d, sums.data(), nullptr, total, nullptr);
    if (q == VC_OK) q = vc_depthcal_fit(d, o.degree, o.min_count, o.min_spread);
    if (q == VC_OK) q = vc_depthcal_get_fit(d, c, a.data(), b.data(), st.data(), rms, nullptr);
    if (q == VC_ERR_NUMERIC) { *err = "no correction can be fitted: " + std::to_string(total[7]) + " pixels of " + std::to_string(n) + " frames see the board"; status = 1; }
    else if (q != VC_OK) { *err = "the fit failed (status " + std::to_string(q) + ")"; status = q == VC_ERR_NO_DEVICE ? 3 : 1; }
  }
  vc_depthcal_destroy(d);
  if (status != 0) return status;
  FILE* fc = std::fopen((o.dir + "/depthcal_cells.csv").c_str(), "w");
  if (!fc) { *err = "cannot write " + o.dir + "/depthcal_cells.csv"; return 1; }
  std::fprintf(fc, "cx,cy,n,sum_x,sum_x2,sum_x3,sum_x4,sum_d,sum_dx,sum_dx2,sum_dd\n");
  for (int k = 0; k < cells; ++k) {
    std::fprintf(fc, "%d,%d", k % o.bx, k / o.bx);
    for (int t = 0; t < 9; ++t) std::fprintf(fc, ",%.17g", sums[(size_t)k * 9 + t]);
    std::fprintf(fc, "\n");
  }
  if (std::fclose(fc) != 0) { *err = "cannot write " + o.dir + "/depthcal_cells.csv in full"; return 1; }
  FILE* fo = std::fopen((o.dir + "/depth_correction.csv").c_str(), "w");
  if (!fo) { *err = "cannot write " + o.dir + "/depth_correction.csv"; return 1; }
  std::fprintf(fo, "size,%d,%d\nbins,%d,%d\nv_ref,%.17g\nunit,%.17g\ndegree,%d\nc,%.17g,%.17g,%.17g\ncx,cy,n,status,a,b\n", S.width, S.height, o.bx, o.by, o.v_ref, o.unit, o.degree,
               c[0], c[1], c[2]);
  int n_status[3] = {0, 0, 0};
  for (int k = 0; k < cells; ++k) {
    std::fprintf(fo, "%d,%d,%.17g,%d,%.17g,%.17g\n", k % o.bx, k / o.bx, sums[(size_t)k * 9], st[k], a[k], b[k]);
    ++n_status[st[k]];
  }
  if (std::fclose(fo) != 0) { *err = "cannot write " + o.dir + "/depth_correction.csv in full"; return 1; }
  std::printf("depth calibration of camera %d (%s) from %zu frames, %lld pixels: rms %.4g counts raw, %.4g after the polynomial, %.4g after the cells; %d cells fitted, "
              "%d with an offset only, %d with too few pixels -> %s\n", o.cam, ModelName(S.model), n, total[7], rms[0], rms[1], rms[2], n_status[0], n_status[1], n_status[2],
              o.dir.c_str());
  return 0;
}
struct DepthCorrectionFile { int w = 0, h = 0, bx = 0, by = 0, degree = 0; double v_ref = 0, unit = 0, c[3] = {0, 0, 0}; std::vector<double> a, b; };
static bool ReadDepthCorrection(const std::string& path, DepthCorrectionFile* f, std::string* err) {
  std::ifstream in(path);
  if (!in) { *err = "cannot open correction file " + path; return false; }
  std::string line;
  bool ok = true;
  auto header = [&](const char* fmt, auto... ptr) { ok = ok && std::getline(in, line) && std::sscanf(line.c_str(), fmt, ptr...) == (int)sizeof...(ptr); };
  header("size,%d,%d", &f->w, &f->h); header("bins,%d,%d", &f->bx, &f->by); header("v_ref,%lf", &f->v_ref); header("unit,%lf", &f->unit); header("degree,%d", &f->degree);
  header("c,%lf,%lf,%lf", &f->c[0], &f->c[1], &f->c[2]);
  ok = ok && std::getline(in, line) && line.compare(0, 5, "cx,cy") == 0;
  if (!ok || f->w < 2 || f->h < 2 || f->w > 8192 || f->h > 8192 || f->bx < 1 || f->by < 1 || f->bx > 32 || f->by > 32 || f->degree < 0 || f->degree > 2 || !(f->v_ref > 0.0) ||
      !(f->unit > 0.0)) { *err = path + ": not a depth correction file"; return false; }
  f->a.assign((size_t)f->bx * f->by, 0.0); f->b = f->a;
  for (int k = 0; k < f->bx * f->by; ++k) {
    int cx, cy, st; double n;
    if (!std::getline(in, line) || std::sscanf(line.c_str(), "%d,%d,%lf,%d,%lf,%lf", &cx, &cy, &n, &st, &f->a[k], &f->b[k]) != 6 || cx != k % f->bx || cy != k / f->bx) {
      *err = path + ": expected the row of cell " + std::to_string(k); return false;
    }
  }
  return true;
}
// Corrects the images of -depthcal_depth with a correction file.  Exit status as above.
static int DepthCalApply(const DepthCalCli& o, int device, std::string* err) {
  DepthCorrectionFile f;
  if (!ReadDepthCorrection(o.file, &f, err)) return 1;
  std::vector<std::string> files;
  if (!GlobSorted(StripScheme(o.depth), &files)) { *err = "no depth image matches " + o.depth; return 1; }
  std::vector<unsigned short> depth;
  if (!ReadDepthFiles(files, f.w, f.h, "the correction", &depth, err)) return 1;
  if (!MakeDir(o.dir, err)) return 1;
  // the correction needs no camera: any camera of the file's size serves the handle
  const double K[4] = {(double)f.w, (double)f.w, 0.5 * (f.w - 1), 0.5 * (f.h - 1)}, T[7] = {0, 0, 0, 1, 0, 0, 0}, rect[4] = {0, 0, 1, 1};
  vc_depthcal* d = nullptr;
  const int st_create = vc_depthcal_create(device, 4 /* linear */, K, 4, f.w, f.h, T, f.unit, 0, rect, f.bx, f.by, f.v_ref, 1.0, 1.0, &d);
  if (st_create == VC_ERR_NO_DEVICE) { *err = "no HIP device (there is no CPU fallback)"; return 3; }
  if (st_create != VC_OK || vc_depthcal_set_fit(d, f.degree, f.c, f.a.data(), f.b.data()) != VC_OK) { vc_depthcal_destroy(d); *err = "the correction file is refused"; return 1; }
  const size_t ns = (size_t)f.w * f.h, n = files.size();
  FILE* csv = std::fopen((o.dir + "/depthcal_apply.csv").c_str(), "w");
  if (!csv) { vc_depthcal_destroy(d); *err = "cannot write " + o.dir + "/depthcal_apply.csv"; return 1; }
  std::fprintf(csv, "image,zero,corrected,out_of_range\n");
  int status = 0;
  long long done = 0, lost = 0;
  for (size_t first = 0; first < n && status == 0; first += 16) {
    const int m = (int)std::min<size_t>(16, n - first);
    long long cnt[3 * 16];
    unsigned short* img = depth.data() + first * ns;
    const int q = vc_depthcal_apply(d, m, img, 2 * f.w, (long long)(2 * ns), img, 2 * f.w, (long long)(2 * ns), o.interp, cnt);
    if (q != VC_OK) { *err = "the correction failed (status " + std::to_string(q) + ")"; status = q == VC_ERR_NO_DEVICE ? 3 : 1; break; }
    for (int k = 0; k < m && status == 0; ++k) {
      const std::string name = BaseName(files[first + k]);
      if (!WritePgm16(o.dir + "/" + name + ".pgm", f.w, f.h, img + k * ns, err)) status = 1;
      std::fprintf(csv, "%s,%lld,%lld,%lld\n", name.c_str(), cnt[3 * k], cnt[3 * k + 1], cnt[3 * k + 2]);
      done += cnt[3 * k + 1]; lost += cnt[3 * k + 2];
    }
  }
  if (std::fclose(csv) != 0 && status == 0) { *err = "cannot write " + o.dir + "/depthcal_apply.csv in full"; status = 1; }
  vc_depthcal_destroy(d);
  if (status != 0) return status;
  std::printf("corrected %zu depth images (%s): %lld values corrected, %lld out of range -> %s\n", n, o.interp ? "bilinear" : "cell", done, lost, o.dir.c_str());
  return 0;
}

// ---- -convert_models / -convert_to: calibrated cameras converted to other camera models (vc_convert*) ------------------------------------
// ---- -allan_imu: the noise of an IMU from a log recorded at rest (vc_allan*) -----------------------------------------------------------
struct AllanCli { bool on = false; std::string imu, dir; int per_decade = 20; double max_fraction = 1.0 / 9.0, window_s = 1.0, gyro_thr = 0.0, accel_thr = 0.0; };
static bool AllanFlags(AllanCli* o, std::string* err) {
  o->imu = FlagString("allan_imu"); o->dir = FlagString("allan_dir");
  o->on = !o->imu.empty();
  if (!o->on && o->dir.empty()) return true;
  if (o->imu.empty() || o->dir.empty()) { *err = "-allan_imu and -allan_dir need each other"; return false; }
  o->per_decade = (int)FlagInt("allan_per_decade"); o->max_fraction = FlagDouble("allan_max_fraction"); o->window_s = FlagDouble("allan_static_window_s");
  o->gyro_thr = FlagDouble("allan_static_gyro"); o->accel_thr = FlagDouble("allan_static_accel");
  if (o->per_decade < 1 || o->per_decade > 1000) { *err = "illegal value for flag 'allan_per_decade': expected 1 ... 1000"; return false; }
  if (!(o->max_fraction > 0.0 && o->max_fraction <= 0.5)) { *err = "illegal value for flag 'allan_max_fraction': expected a fraction in (0, 0.5]"; return false; }
  if (!(o->window_s > 0.0) || !std::isfinite(o->window_s)) { *err = "illegal value for flag 'allan_static_window_s': expected a positive number of seconds"; return false; }
  if (std::isnan(o->gyro_thr) || std::isnan(o->accel_thr)) { *err = "illegal value for flag 'allan_static_gyro' / 'allan_static_accel': not a number"; return false; }
  return true;
}
// Exit status: 0, 1 (an error said in *err) or 3 (no device).
static int AllanImu(const AllanCli& o, int device, std::string* err) {
  static const char* kAxis[6] = {"gx", "gy", "gz", "ax", "ay", "az"};
  ImuData imu;
  if (!ReadImu(StripScheme(o.imu), FlagBool("use_system_time"), &imu, err)) return 1;
  const size_t n = imu.time.size();
  if (n < 2) { *err = "the log " + o.imu + " holds fewer than two samples"; return 1; }
  if (n > (size_t)vc::kAllanMaxN) { *err = "the log holds more than 2^24 samples"; return 1; }
  if (!MakeDir(o.dir, err)) return 1;
  vc_allan* raw = nullptr;
  const int st_create = vc_allan_create(device, (int)n, imu.gyro.data(), imu.accel.data(), imu.time.data(), &raw);
  if (st_create == VC_ERR_NO_DEVICE) { *err = "no HIP device (there is no CPU fallback)"; return 3; }
  if (st_create != VC_OK) { *err = "the log was refused: a sample or a time stamp is not finite (status " + std::to_string(st_create) + ")"; return 1; }
  std::unique_ptr<vc_allan, void (*)(vc_allan*)> a(raw, vc_allan_destroy);
  double tau0 = 0.0, dt_min = 0.0, dt_max = 0.0, means[6];
  long long irregular = 0;
  int range[2] = {0, (int)n};
  vc_allan_get(a.get(), nullptr, &tau0, &dt_min, &dt_max, means, &irregular, range);
  if (o.gyro_thr > 0.0 || o.accel_thr > 0.0) {
    const long window = std::max(1L, std::lround(o.window_s / tau0));
    if (2 * window >= (long)n) { *err = "-allan_static_window_s: two windows of " + std::to_string(window) + " samples do not fit into the log"; return 1; }
    int n_quiet = 0;
    const int q = vc_allan_static(a.get(), (int)window, o.gyro_thr, o.accel_thr, range, &n_quiet);
    if (q == 1) { *err = "no window of " + std::to_string(window) + " samples is quiet under -allan_static_gyro / -allan_static_accel"; return 1; }
    if (q != VC_OK) { *err = "the quiet test failed (status " + std::to_string(q) + ")"; return q == VC_ERR_NO_DEVICE ? 3 : 1; }
    std::fprintf(stderr, "I static stretch: samples %d ... %d of %zu (%.1f s), %d quiet window starts of %ld samples\n", range[0], range[0] + range[1] - 1, n,
                 range[1] * tau0, n_quiet, window);
  }
  vic::AllanFactors f;
  vic::AllanCurve curve;
  try { f = vic::AllanFactorList(range[1], o.per_decade, o.max_fraction); }
  catch (const std::exception& e) { *err = e.what(); return 1; }
  const size_t n_m = f.m.size();
  curve.avar.resize(6 * n_m); curve.terms.resize(n_m);
  const int q = vc_allan_run(a.get(), (int)n_m, f.m.data(), curve.avar.data(), curve.terms.data());
  if (q != VC_OK) { *err = "the sweep failed (status " + std::to_string(q) + ")"; return q == VC_ERR_NO_DEVICE ? 3 : 1; }
  std::vector<double> tau(n_m);
  for (size_t j = 0; j < n_m; ++j) tau[j] = f.m[j] * tau0;
  vic::AllanFitResult fit[6];
  for (int c = 0; c < 6; ++c) fit[c] = vic::AllanFit(tau, curve.avar.data() + c * n_m, f.rel_err);
  // ---- allan.csv: one line per averaging time
  {
    std::ofstream out(o.dir + "/allan.csv");
    if (!out) { *err = "cannot write " + o.dir + "/allan.csv"; return 1; }
    out << "tau,m,terms,rel_err";
    for (int c = 0; c < 6; ++c) out << ",adev_" << kAxis[c];
    for (int c = 0; c < 6; ++c) out << ",model_" << kAxis[c];
    out << "\n";
    char buf[64];
    for (size_t j = 0; j < n_m; ++j) {
      std::snprintf(buf, sizeof(buf), "%.10e,%d,%d,%.10e", tau[j], f.m[j], curve.terms[j], f.rel_err[j]); out << buf;
      for (int c = 0; c < 6; ++c) { std::snprintf(buf, sizeof(buf), ",%.10e", std::sqrt(curve.avar[c * n_m + j])); out << buf; }
      for (int c = 0; c < 6; ++c) {
        const double md = fit[c].status == 0 ? std::sqrt(vc::allan_model(fit[c].N, fit[c].B, fit[c].K, tau[j])) : std::nan("");
        std::snprintf(buf, sizeof(buf), ",%.10e", md); out << buf;
      }
      out << "\n";
    }
  }
  // ---- allan_summary.csv: one line per axis; sigma = N / sqrt(tau0), the per-sample standard deviation at the log's own rate
  const double sqrt_tau0 = std::sqrt(tau0);
  {
    std::ofstream out(o.dir + "/allan_summary.csv");
    if (!out) { *err = "cannot write " + o.dir + "/allan_summary.csv"; return 1; }
    out << "axis,mean,adev_tau0,N,B,K,active_terms,fit_rms_log,fit_status,sigma,n,first,count,tau0,irregular_intervals\n";
    char buf[400];
    for (int c = 0; c < 6; ++c) {
      std::snprintf(buf, sizeof(buf), "%s,%.10e,%.10e,%.10e,%.10e,%.10e,%s%s%s,%.6e,%d,%.10e,%zu,%d,%d,%.10e,%lld\n", kAxis[c], means[c], std::sqrt(curve.avar[c * n_m]),
                    fit[c].N, fit[c].B, fit[c].K, (fit[c].mask & 1) ? "N" : "", (fit[c].mask & 2) ? "B" : "", (fit[c].mask & 4) ? "K" : "", fit[c].rms_log,
                    fit[c].status, fit[c].N / sqrt_tau0, n, range[0], range[1], tau0, irregular);
      out << buf;
    }
  }
  // ---- what the user reads
  double sigma[2] = {0.0, 0.0};
  bool have[2] = {false, false};
  for (int s = 0; s < 2; ++s) {
    double q2 = 0.0; int used = 0;
    for (int c = 3 * s; c < 3 * s + 3; ++c) {
      if (fit[c].status != 0) { std::fprintf(stderr, "W the fit of axis %s failed (status %d): it is left out of its sensor's sigma\n", kAxis[c], fit[c].status); continue; }
      q2 += fit[c].N * fit[c].N; ++used;
    }
    if (used > 0) { sigma[s] = std::sqrt(q2 / used) / sqrt_tau0; have[s] = true; }
    std::fprintf(stderr, "I %s white noise N = %.6e %.6e %.6e %s/sqrt(Hz) (x y z)\n", s == 0 ? "gyro" : "accel", fit[3 * s].N, fit[3 * s + 1].N, fit[3 * s + 2].N,
                 s == 0 ? "rad/s" : "m/s^2");
  }
  if ((double)irregular > 0.01 * (double)(n - 1))
    std::fprintf(stderr, "W %lld of %zu intervals lie outside [0.5, 1.5] tau0 (tau0 = %.6g s, %.6g ... %.6g s): the log is not resampled\n", irregular, n - 1, tau0, dt_min, dt_max);
  if (range[1] * tau0 < 100.0) std::fprintf(stderr, "W the range used is %.1f s long: under 100 s the long averaging times carry little\n", range[1] * tau0);
  if (have[0] && have[1]) std::printf("-gyro_sigma %.8e -accel_sigma %.8e\n", sigma[0], sigma[1]);
  else std::fprintf(stderr, "W no sigma for a sensor without a fitted axis: nothing to paste\n");
  std::fprintf(stderr, "I wrote %s/allan.csv (%zu averaging times) and %s/allan_summary.csv\n", o.dir.c_str(), n_m, o.dir.c_str());
  return 0;
}

static const char* ModelXmlType(int id) {
  static const char* n[] = {"calibu_fu_fv_u0_v0_w", "calibu_fu_fv_u0_v0_k1_k2", "calibu_fu_fv_u0_v0_k1_k2_k3", "calibu_fu_fv_u0_v0_kb4", "calibu_fu_fv_u0_v0", "calibu_fu_fv_u0_v0_rational6"};
  return (id >= 0 && id < 6) ? n[id] : "?";
}
struct ConvertOptions { std::string output; std::vector<int> models; int gx = 64, gy = 48; double fit_radius = 1.0; };
// the flags of a conversion, checked before anything else runs
static bool ConvertFlags(ConvertOptions* o, std::string* err) {
  const std::string to = FlagString("convert_to");
  if (to.empty()) { *err = "-convert_models needs -convert_to"; return false; }
  o->models.clear();
  for (size_t from = 0; from <= to.size();) {
    const size_t comma = std::min(to.find(',', from), to.size());
    const std::string name = to.substr(from, comma - from);
    const int id = ModelId(name);
    if (id < 0) { *err = "illegal value '" + to + "' specified for flag 'convert_to': expected fov, poly2, poly3, kb4, linear or rational6, one for all cameras or one per camera"; return false; }
    o->models.push_back(id);
    from = comma + 1;
  }
  o->output = FlagString("convert_output");
  if (o->output.empty()) { *err = "illegal value for flag 'convert_output': expected a file name"; return false; }
  if (!ParseCompareGrid(FlagString("convert_grid"), &o->gx, &o->gy)) { *err = "illegal value '" + FlagString("convert_grid") + "' specified for flag 'convert_grid': expected GXxGY, both at least 2, at most 2^22 samples"; return false; }
  o->fit_radius = FlagDouble("convert_fit_radius");
  if (!(o->fit_radius > 0.0 && o->fit_radius <= 1e6)) { *err = "illegal value for flag 'convert_fit_radius': expected a radius above 0"; return false; }
  return true;
}
// what can be said about the cameras before a device is looked for
static bool ConvertibleRig(const std::vector<vic::CameraAndPose>& cams, const ConvertOptions& o, std::string* err) {
  if (o.models.size() != 1 && o.models.size() != cams.size()) {
    *err = "illegal value for flag 'convert_to': " + std::to_string(o.models.size()) + " models for " + std::to_string(cams.size()) + " cameras (expected one, or one per camera)"; return false;
  }
  for (size_t c = 0; c < cams.size(); ++c)
    if (o.gx > cams[c].width || o.gy > cams[c].height) { *err = "camera " + std::to_string(c) + ": -convert_grid exceeds the image"; return false; }
  return true;
}
// Converts the cameras of the rig file `path` (read into `cams`) and writes -convert_output: the file's own text with every camera's model type and
// <params> replaced -- poses, sizes and axes stay as they are written.  Then, with `compare`, the comparison of the original against the
// converted cameras.  Exit status: 0, 1 (an error said in *err, or a camera whose fit failed) or 3 (no device).
static int ConvertRig(const std::string& path, const std::vector<vic::CameraAndPose>& cams, const ConvertOptions& o, const CompareOptions* compare, int device, std::string* err) {
  if (!ConvertibleRig(cams, o, err)) return 1;
  std::ifstream f(path);
  if (!f) { *err = "cannot open rig file " + path; return 1; }
  std::stringstream ss; ss << f.rdbuf();
  std::string text = ss.str();
  std::vector<vic::CameraAndPose> converted = cams;
  std::vector<std::string> lines;
  bool failed = false;
  size_t from = 0;
  for (size_t c = 0; c < cams.size(); ++c) {
    const int model_b = o.models[o.models.size() == 1 ? 0 : c];
    vc_converter* h = nullptr;
    const int st_create = vc_converter_create(device, cams[c].model, cams[c].params.data(), (int)cams[c].params.size(), cams[c].width, cams[c].height, model_b, o.gx, o.gy, &h);
    if (st_create == VC_ERR_NO_DEVICE) { *err = "no HIP device (there is no CPU fallback)"; return 3; }
    if (st_create != VC_OK) { *err = "camera " + std::to_string(c) + ": the conversion refuses this camera (status " + std::to_string(st_create) + ")"; return 1; }
    vic::ConvertResult r;
    int nk = 0;
    r.params.resize(10);
    int q = vc_convert_run(h, o.fit_radius, 200, nullptr, 0);
    if (q == VC_OK) q = vc_convert_get(h, r.params.data(), &nk, &r.status, &r.iterations, &r.n_fit, &r.n_left_out, &r.cost0, &r.cost, &r.max_err, &r.worst);
    vc_converter_destroy(h);
    if (q != VC_OK) {
      *err = "camera " + std::to_string(c) + (q == VC_ERR_NUMERIC ? ": the target model cannot be fitted (too few samples within -convert_fit_radius that the camera has a ray for, or a start nothing can be evaluated at)"
                                                                  : ": the conversion failed (status " + std::to_string(q) + ")");
      return q == VC_ERR_NO_DEVICE ? 3 : 1;
    }
    r.params.resize((size_t)nk);
    converted[c].model = model_b; converted[c].params = r.params;
    if (r.status == 2) failed = true;
    const int used = r.n_fit - r.n_left_out;
    char line[256];
    std::snprintf(line, sizeof(line), "camera %zu: %s converted to %s: status %d, %d iterations, %.6g px rms, %.6g px max over %d samples", c, ModelName(cams[c].model),
                  ModelName(model_b), r.status, r.iterations, used > 0 ? std::sqrt(2.0 * r.cost / used) : 0.0, r.max_err, used);
    lines.push_back(line);
    // the c-th <camera> of the text: its type and its parameters
    const size_t p = text.find("<camera>", from), e = p == std::string::npos ? p : text.find("</camera>", p);
    const size_t t0 = p == std::string::npos ? p : text.find("type=\"", p), a0 = p == std::string::npos ? p : text.find("<params>", p);
    const size_t t1 = t0 == std::string::npos ? t0 : text.find('"', t0 + 6), a1 = a0 == std::string::npos ? a0 : text.find("</params>", a0);
    if (e == std::string::npos || t1 == std::string::npos || a1 == std::string::npos || t1 > e || a1 > e || t1 > a0) { *err = path + ": camera " + std::to_string(c) + " cannot be rewritten"; return 1; }
    std::string params = "<params> [ ";
    for (int k = 0; k < nk; ++k) { char num[40]; std::snprintf(num, sizeof(num), "%.17g", r.params[k]); params += num; params += k + 1 < nk ? "; " : " ] "; }
    text.replace(a0, a1 - a0, params);                            // (the later position first: the earlier one stays valid)
    text.replace(t0 + 6, t1 - t0 - 6, ModelXmlType(model_b));
    from = text.find("</camera>", p) + 9;
  }
  std::ofstream out(o.output);
  out << text;
  out.close();
  if (!out) { *err = "cannot write " + o.output; return 1; }
  for (const std::string& l : lines) std::printf("%s\n", l.c_str());
  std::printf("conversion %s -> %s\n", failed ? "FAILED" : "succeeded", o.output.c_str());
  if (compare) {
    const int rc = CompareRigs(cams, converted, *compare, device, err);
    if (rc != 0) return rc;
  }
  if (failed) { *err = "a camera's fit failed (status 2): its parameters are the last accepted point"; return 1; }
  return 0;
}

// ---- -uncertainty_dir: the projection uncertainty of every camera just calibrated, mapped over its image (vc_uncertainty*) -----------------
struct UncertaintyOptions { std::string dir; int gx = 64, gy = 48, rings = 8; double fit_radius = 0.5, noise = 0.0; };
static bool UncertaintyFlags(UncertaintyOptions* o, std::string* err) {
  o->dir = FlagString("uncertainty_dir");
  if (!ParseCompareGrid(FlagString("uncertainty_grid"), &o->gx, &o->gy)) { *err = "illegal value '" + FlagString("uncertainty_grid") + "' specified for flag 'uncertainty_grid': expected GXxGY, both at least 2, at most 2^22 samples"; return false; }
  o->fit_radius = FlagDouble("uncertainty_fit_radius");
  if (!(std::fabs(o->fit_radius) <= 1e6)) { *err = "illegal value for flag 'uncertainty_fit_radius': expected a finite radius"; return false; }
  o->rings = (int)FlagInt("uncertainty_rings");
  if (o->rings < 1 || o->rings > 64) { *err = "illegal value for flag 'uncertainty_rings': expected 1 ... 64"; return false; }
  o->noise = FlagDouble("uncertainty_noise");
  if (!(o->noise >= 0.0 && o->noise <= 1e6)) { *err = "illegal value for flag 'uncertainty_noise': expected 0 (the camera's own RMSE) or a noise in px above 0"; return false; }
  return true;
}
// cov: the solution covariance (dim x dim, blocks q_ck (4), p_ck (3), params (nk) per camera); cams: model, params and size of every camera;
// rmse: the cameras' reprojection RMSE per coordinate.  Writes the files of -uncertainty_dir and prints one line per camera.
static bool UncertaintyOutputs(const std::vector<vic::CameraAndPose>& cams, const std::vector<double>& cov, int dim, const std::vector<double>& rmse,
                               const UncertaintyOptions& o, int device, std::string* err) {
  struct stat st;
  if (mkdir(o.dir.c_str(), 0777) != 0 && !(stat(o.dir.c_str(), &st) == 0 && S_ISDIR(st.st_mode))) { *err = "cannot create the directory " + o.dir; return false; }      // (one level)
  FILE* fs = std::fopen((o.dir + "/uncertainty_summary.csv").c_str(), "w");
  if (!fs) { *err = "cannot write into " + o.dir; return false; }
  std::fprintf(fs, "camera,ring,rho_from,rho_to,count,invalid,rms_px,max_sigma_px,noise_px\n");
  std::vector<std::vector<double>> blocks(cams.size());
  bool ok = true;
  int first = 0;
  for (size_t c = 0; c < cams.size() && ok; ++c) {
    const int nk = (int)cams[c].params.size();
    first += 7;
    if (first + nk > dim) { *err = "the solution covariance has no block for the intrinsics of camera " + std::to_string(c); ok = false; break; }
    std::vector<double>& block = blocks[c];
    block.resize((size_t)nk * nk);
    for (int r = 0; r < nk; ++r) for (int q = 0; q < nk; ++q) block[(size_t)r * nk + q] = cov[(size_t)(first + r) * dim + first + q];
    first += nk;
    const double noise = o.noise > 0.0 ? o.noise : rmse[c];
    vc_uncertainty* h = nullptr;
    int q = vc_uncertainty_create(device, cams[c].model, cams[c].params.data(), nk, cams[c].width, cams[c].height, o.gx, o.gy, &h);
    const size_t n = (size_t)o.gx * o.gy;
    std::vector<double> sg(3 * n);
    std::vector<unsigned char> fl(n);
    vic::UncertaintySummary s;
    vic::UncertaintyRings r;
    r.count.resize(o.rings); r.invalid.resize(o.rings); r.sum_var.resize(o.rings); r.max_lam.resize(o.rings);
    if (q == VC_OK) q = vc_uncertainty_run(h, block.data(), noise, o.fit_radius);
    if (q == VC_OK) q = vc_uncertainty_get_map(h, sg.data(), fl.data());
    if (q == VC_OK) q = vc_uncertainty_summary(h, &s.count, &s.invalid, &s.sum_var, &s.max_lam, &s.worst);
    if (q == VC_OK) q = vc_uncertainty_rings(h, o.rings, r.count.data(), r.invalid.data(), r.sum_var.data(), r.max_lam.data());
    vc_uncertainty_destroy(h);
    if (q != VC_OK) {
      *err = "camera " + std::to_string(c) + (q == VC_ERR_NUMERIC ? ": the absorbed rotation cannot be fitted (fewer than 3 samples within -uncertainty_fit_radius, or a degenerate system)"
                                                                  : q == VC_ERR_BAD_ARG && !(noise > 0.0) ? ": the noise is 0 (a reprojection RMSE of 0: give -uncertainty_noise)"
                                                                  : ": the uncertainty map failed (status " + std::to_string(q) + ")");
      ok = false; break;
    }
    FILE* fm = std::fopen((o.dir + "/uncertainty_cam" + std::to_string(c) + ".csv").c_str(), "w");
    if (!fm) { *err = "cannot write into " + o.dir; ok = false; break; }
    std::fprintf(fm, "x,y,s_uu,s_uv,s_vv,sigma_max,flags\n");
    for (size_t k = 0; k < n; ++k) {
      const int i = (int)(k % o.gx), j = (int)(k / o.gx);
      const double* t = &sg[3 * k];
      const double df = t[0] - t[2], lam = 0.5 * ((t[0] + t[2]) + std::sqrt(df * df + 4.0 * (t[1] * t[1])));
      std::fprintf(fm, "%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%d\n", (double)(i * (cams[c].width - 1)) / (o.gx - 1), (double)(j * (cams[c].height - 1)) / (o.gy - 1), t[0], t[1], t[2],
                   std::sqrt(lam > 0.0 ? lam : lam == lam ? 0.0 : lam), (int)fl[k]);
    }
    std::fclose(fm);
    for (int k = 0; k < o.rings; ++k)
      std::fprintf(fs, "%zu,%d,%.17g,%.17g,%lld,%lld,%.17g,%.17g,%.17g\n", c, k, (double)k / o.rings, (double)(k + 1) / o.rings, r.count[k], r.invalid[k],
                   r.count[k] > 0 ? std::sqrt(r.sum_var[k] / r.count[k]) : 0.0, std::sqrt(r.max_lam[k]), noise);
    if (s.worst >= 0)
      std::printf("camera %zu: projection uncertainty: worst sigma_max %.4g px at (%.1f, %.1f), %.4g px rms expected shift over %lld samples, noise %.4g px\n", c,
                  std::sqrt(s.max_lam), (double)((s.worst % o.gx) * (cams[c].width - 1)) / (o.gx - 1), (double)((s.worst / o.gx) * (cams[c].height - 1)) / (o.gy - 1),
                  std::sqrt(s.sum_var / s.count), s.count, noise);
    else std::printf("camera %zu: projection uncertainty: no valid sample\n", c);
  }
  if (ok) {                                              // the second table: the covariance of the intrinsics that was mapped, row by row
    std::fprintf(fs, "camera,parameter,covariance\n");
    for (size_t c = 0; c < cams.size(); ++c) {
      const int nk = (int)cams[c].params.size();
      for (int r = 0; r < nk; ++r) {
        std::fprintf(fs, "%zu,%d", c, r);
        for (int q = 0; q < nk; ++q) std::fprintf(fs, ",%.17g", blocks[c][(size_t)r * nk + q]);
        std::fprintf(fs, "\n");
      }
    }
  }
  std::fclose(fs);
  return ok;
}

// ---- -stereo_uncertainty_dir: the row and depth uncertainty of two cameras just calibrated, mapped over the rectified image (vc_stereo_uncertainty*)
struct StereoUncertaintyOptions { std::string dir; int a = 0, b = 1, gx = 64, gy = 48; std::vector<double> depths; double noise = 0.0, alpha = 0.0; };
static bool StereoUncertaintyFlags(StereoUncertaintyOptions* o, std::string* err) {
  o->dir = FlagString("stereo_uncertainty_dir");
  if (!ParseCompareGrid(FlagString("stereo_uncertainty_grid"), &o->gx, &o->gy)) { *err = "illegal value '" + FlagString("stereo_uncertainty_grid") + "' specified for flag 'stereo_uncertainty_grid': expected GXxGY, both at least 2, at most 2^22 samples"; return false; }
  char tail = 0;
  if (std::sscanf(FlagString("stereo_uncertainty_cams").c_str(), "%d,%d%c", &o->a, &o->b, &tail) != 2 || o->a < 0 || o->b < 0 || o->a == o->b) {
    *err = "illegal value '" + FlagString("stereo_uncertainty_cams") + "' specified for flag 'stereo_uncertainty_cams': expected a,b, two different cameras";
    return false;
  }
  std::stringstream ss(FlagString("stereo_uncertainty_depths"));
  std::string item;
  while (std::getline(ss, item, ',')) {
    char* end = nullptr;
    const double z = std::strtod(item.c_str(), &end);
    if (item.empty() || end != item.c_str() + item.size() || !(z > 0.0) || !(z <= 1e300)) { o->depths.clear(); break; }
    o->depths.push_back(z);
  }
  if (o->depths.empty() || o->depths.size() > 8) { *err = "illegal value '" + FlagString("stereo_uncertainty_depths") + "' specified for flag 'stereo_uncertainty_depths': expected 1 ... 8 depths above 0, separated by commas"; return false; }
  o->noise = FlagDouble("stereo_uncertainty_noise");
  if (!(o->noise >= 0.0 && o->noise <= 1e6)) { *err = "illegal value for flag 'stereo_uncertainty_noise': expected 0 (the two cameras' mean RMSE) or a noise in px above 0"; return false; }
  o->alpha = FlagDouble("rectify_alpha");
  if (!o->dir.empty() && !(o->alpha >= 0.0 && o->alpha <= 1.0)) { *err = "illegal value for flag 'rectify_alpha': expected 0 ... 1"; return false; }
  return true;
}
// cov: the solution covariance (dim x dim, blocks q_ck (4), p_ck (3), params (nk) per camera); cams: model, params, size and pose of every camera;
// rmse: the cameras' reprojection RMSE per coordinate.  Writes the files of -stereo_uncertainty_dir and prints one line per depth.
static bool StereoUncertaintyOutputs(const std::vector<vic::CameraAndPose>& cams, const std::vector<double>& cov, int dim, const std::vector<double>& rmse,
                                     const StereoUncertaintyOptions& o, int device, std::string* err) {
  const vic::CameraAndPose& A = cams[o.a];
  const vic::CameraAndPose& B = cams[o.b];
  std::vector<int> idx;
  for (int s = 0; s < 2; ++s) {
    const int c = s ? o.b : o.a;
    int first = 0;
    for (int k = 0; k < c; ++k) first += 7 + (int)cams[k].params.size();
    for (int k = 0; k < 7 + (int)cams[c].params.size(); ++k) idx.push_back(first + k);
    if (first + 7 + (int)cams[c].params.size() > dim) { *err = "the solution covariance has no blocks for camera " + std::to_string(c); return false; }
  }
  const size_t m = idx.size();
  std::vector<double> block(m * m);
  for (size_t r = 0; r < m; ++r) for (size_t q = 0; q < m; ++q) block[r * m + q] = cov[(size_t)idx[r] * dim + idx[q]];
  const double noise = o.noise > 0.0 ? o.noise : 0.5 * (rmse[o.a] + rmse[o.b]);
  const int nd = (int)o.depths.size();
  const size_t n = (size_t)o.gx * o.gy;
  std::vector<double> var(3 * n * nd);
  std::vector<unsigned char> fl(n * nd);
  std::vector<vic::StereoUncertaintySummary> sum((size_t)nd);
  double dl[4] = {0, 0, 0, 0}, baseline = 0.0, pose_var[7] = {0, 0, 0, 0, 0, 0, 0};
  vc_stereo_uncertainty* h = nullptr;
  int q = vc_stereo_uncertainty_create(device, A.model, A.params.data(), (int)A.params.size(), A.width, A.height, A.T_ck.data(), B.model, B.params.data(), (int)B.params.size(),
                                       B.width, B.height, B.T_ck.data(), nullptr, A.width, A.height, o.alpha, o.gx, o.gy, &h);
  if (q == VC_OK) q = vc_stereo_uncertainty_run(h, block.data(), noise, o.depths.data(), nd);
  if (q == VC_OK) q = vc_stereo_uncertainty_get_map(h, var.data(), fl.data());
  for (int k = 0; k < nd && q == VC_OK; ++k)
    q = vc_stereo_uncertainty_summary(h, k, &sum[k].count, &sum[k].invalid, &sum[k].sum_var_dv, &sum[k].sum_var_d, &sum[k].sum_var_z, &sum[k].max_var_dv, &sum[k].worst);
  if (q == VC_OK) q = vc_stereo_uncertainty_get_pose_sigma(h, pose_var);
  if (q == VC_OK) q = vc_stereo_uncertainty_get(h, nullptr, nullptr, dl, &baseline, nullptr);
  vc_stereo_uncertainty_destroy(h);
  if (q != VC_OK) {
    *err = q == VC_ERR_NUMERIC ? "the two cameras' centres coincide, or no destination camera can be fitted"
         : q == VC_ERR_UNSUPPORTED ? "the baseline is vertical: column rectification is not supported"
         : q == VC_ERR_BAD_ARG && !(noise > 0.0) ? "the noise is 0 (a reprojection RMSE of 0: give -stereo_uncertainty_noise)"
         : "the stereo uncertainty map failed (status " + std::to_string(q) + ")";
    return false;
  }
  struct stat st;
  if (mkdir(o.dir.c_str(), 0777) != 0 && !(stat(o.dir.c_str(), &st) == 0 && S_ISDIR(st.st_mode))) { *err = "cannot create the directory " + o.dir; return false; }      // (one level)
  FILE* fm = std::fopen((o.dir + "/stereo_uncertainty.csv").c_str(), "w");
  FILE* fs = fm ? std::fopen((o.dir + "/stereo_uncertainty_summary.csv").c_str(), "w") : nullptr;
  if (!fs) { if (fm) std::fclose(fm); *err = "cannot write into " + o.dir; return false; }
  auto sigma = [](double v) { return std::sqrt(v > 0.0 ? v : v == v ? 0.0 : v); };          // (a rounding below zero is zero; NaN stays)
  auto at_x = [&](long long s) { return (double)((s % o.gx) * (A.width - 1)) / (o.gx - 1); };
  auto at_y = [&](long long s) { return (double)((s / o.gx) * (A.height - 1)) / (o.gy - 1); };
  std::fprintf(fm, "depth,x,y,sigma_dv,sigma_d,sigma_Z,flags\n");
  for (int k = 0; k < nd; ++k)
    for (size_t s = 0; s < n; ++s) {
      const double* t = &var[3 * (k * n + s)];
      std::fprintf(fm, "%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%d\n", o.depths[k], at_x((long long)s), at_y((long long)s), sigma(t[0]), sigma(t[1]), sigma(t[2]), (int)fl[k * n + s]);
    }
  std::fclose(fm);
  std::fprintf(fs, "depth,count,invalid,rms_sigma_dv,max_sigma_dv,worst_x,worst_y,rms_sigma_d,rms_sigma_z_over_z\n");
  for (int k = 0; k < nd; ++k) {
    const vic::StereoUncertaintySummary& s = sum[k];
    const double c = s.count > 0 ? (double)s.count : 1.0;
    std::fprintf(fs, "%.17g,%lld,%lld,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g\n", o.depths[k], s.count, s.invalid, sigma(s.sum_var_dv / c), sigma(s.max_var_dv),
                 s.worst >= 0 ? at_x(s.worst) : -1.0, s.worst >= 0 ? at_y(s.worst) : -1.0, sigma(s.sum_var_d / c), sigma(s.sum_var_z / c) / o.depths[k]);
    if (s.worst >= 0)
      std::printf("cameras %d,%d at %.4g m: row misalignment sigma %.4g px rms, worst %.4g px at (%.1f, %.1f); disparity sigma %.4g px rms; depth sigma %.4g %% rms over %lld samples\n",
                  o.a, o.b, o.depths[k], sigma(s.sum_var_dv / c), sigma(s.max_var_dv), at_x(s.worst), at_y(s.worst), sigma(s.sum_var_d / c), 100.0 * sigma(s.sum_var_z / c) / o.depths[k], s.count);
    else std::printf("cameras %d,%d at %.4g m: stereo uncertainty: no valid sample\n", o.a, o.b, o.depths[k]);
  }
  // the second table: the pair's geometry and the noise; the third: the two cameras that were mapped; the fourth: their covariance, row by row
  // (q_a p_a K_a q_b p_b K_b)
  std::fprintf(fs, "baseline,sigma_baseline,noise_px,fu,fv,u0,v0,width,height\n");
  std::fprintf(fs, "%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%d,%d\n", baseline, sigma(pose_var[6]), noise, dl[0], dl[1], dl[2], dl[3], A.width, A.height);
  std::fprintf(fs, "camera,qx,qy,qz,qw,tx,ty,tz,params\n");
  for (int s = 0; s < 2; ++s) {
    const vic::CameraAndPose& cm = s ? B : A;
    std::fprintf(fs, "%d", s ? o.b : o.a);
    for (int k = 0; k < 7; ++k) std::fprintf(fs, ",%.17g", cm.T_ck.data()[k]);
    for (double p : cm.params) std::fprintf(fs, ",%.17g", p);
    std::fprintf(fs, "\n");
  }
  std::fprintf(fs, "row,covariance\n");
  for (size_t r = 0; r < m; ++r) {
    std::fprintf(fs, "%zu", r);
    for (size_t c = 0; c < m; ++c) std::fprintf(fs, ",%.17g", block[r * m + c]);
    std::fprintf(fs, "\n");
  }
  std::fclose(fs);
  std::printf("cameras %d,%d: baseline %.6g m, sigma %.3g m, noise %.4g px\n", o.a, o.b, baseline, sigma(pose_var[6]), noise);
  return true;
}

// ---- -select_views K -select_dir DIR: the most informative of the calibrated frames (vc_selector*) -----------------------------------------
struct SelectOptions { int k = 0; std::string dir; double prior = 1e-6; std::vector<long> start; };
static bool SelectFlags(SelectOptions* o, std::string* err) {
  const std::string k = FlagString("select_views");
  o->dir = FlagString("select_dir");
  if (k.empty()) {
    if (!o->dir.empty() || !FlagString("select_start").empty()) { *err = "-select_dir and -select_start need -select_views"; return false; }
    return true;
  }
  char* end = nullptr;
  const long kv = std::strtol(k.c_str(), &end, 10);
  if (end == k.c_str() || *end != '\0' || kv < 1 || kv > (1 << 30)) { *err = "illegal value '" + k + "' specified for flag 'select_views': expected a number of views >= 1"; return false; }
  o->k = (int)kv;
  if (o->dir.empty()) { *err = "-select_views needs -select_dir"; return false; }
  if (FlagInt("gpus") > 1) { *err = "-select_views needs -gpus 1: the selection runs over the frames of one calibrator"; return false; }
  {
    std::string parent = o->dir;
    while (parent.size() > 1 && parent.back() == '/') parent.pop_back();
    const size_t slash = parent.rfind('/');
    parent = slash == std::string::npos ? "." : (slash == 0 ? "/" : parent.substr(0, slash));
    struct stat st;
    if (!(stat(parent.c_str(), &st) == 0 && S_ISDIR(st.st_mode))) { *err = "the parent directory of -select_dir " + o->dir + " does not exist"; return false; }
  }
  o->prior = FlagDouble("select_prior");
  if (!(o->prior > 0.0 && o->prior < 1e300)) { *err = "illegal value for flag 'select_prior': expected a finite prior > 0"; return false; }
  for (const std::string& tok : Split(FlagString("select_start"), ',')) {
    const long f = std::strtol(tok.c_str(), &end, 10);
    if (tok.empty() || end == tok.c_str() || *end != '\0' || f < 0) { *err = "illegal value '" + FlagString("select_start") + "' specified for flag 'select_start': expected f0,f1,..."; return false; }
    o->start.push_back(f);
  }
  return true;
}
// The held-out set as the scoring left it (-holdout_every): its tiles, the refitted poses and their status.
struct SelectHeld { std::vector<int> tile_frame, tile_cam, point_id, status; std::vector<long long> tile_off; std::vector<double> points, T_wk; };
// Writes the files of -select_dir and prints one line.  frame_ids: the recording's number of every calibrated frame; held_ids / held: the same of the
// held-out frames, empty without -holdout_every.
static bool SelectOutputs(vic::ViCalibrator& cal, const std::vector<long>& frame_ids, const std::vector<long>& held_ids, const SelectHeld& held, const SelectOptions& o,
                          std::string* err) {
  struct stat st;
  if (mkdir(o.dir.c_str(), 0777) != 0 && !(stat(o.dir.c_str(), &st) == 0 && S_ISDIR(st.st_mode))) { *err = "cannot create the directory " + o.dir; return false; }
  const int N = (int)frame_ids.size();
  std::vector<int> start;
  for (long f : o.start) {
    const auto it = std::find(frame_ids.begin(), frame_ids.end(), f);
    if (it == frame_ids.end() || std::find(start.begin(), start.end(), (int)(it - frame_ids.begin())) != start.end()) {
      *err = "-select_start: frame " + std::to_string(f) + " is not one of the calibrated frames, or is given twice"; return false;
    }
    start.push_back((int)(it - frame_ids.begin()));
  }
  vic::Selector sel(cal);
  sel.Run(1, start, o.prior);
  const std::vector<double> first = sel.LastGains();
  const vic::Selection r = sel.Run(o.k, start, o.prior);
  const vic::SelectionFrames fr = sel.Frames();
  FILE* f = std::fopen((o.dir + "/selected_views.csv").c_str(), "w");
  if (!f) { *err = "cannot write into " + o.dir; return false; }
  std::fprintf(f, "rank,frame,gain,cum,share\n");
  int n90 = 0, n99 = 0;
  for (size_t k = 0; k < r.order.size(); ++k) {
    const double share = r.total > 0.0 ? std::min(1.0, r.cum[k] / r.total) : 1.0;
    if (!n90 && share >= 0.90) n90 = (int)k + 1;
    if (!n99 && share >= 0.99) n99 = (int)k + 1;
    std::fprintf(f, "%zu,%ld,%.10g,%.10g,%.10g\n", k + 1, frame_ids[(size_t)r.order[k]], r.gain[k], r.cum[k], share);
  }
  std::fclose(f);
  f = std::fopen((o.dir + "/select_frames.csv").c_str(), "w");
  if (!f) { *err = "cannot write into " + o.dir; return false; }
  std::fprintf(f, "frame,status,corners,behind,first_round_gain\n");
  int usable = 0;
  for (int i = 0; i < N; ++i) {
    usable += fr.status[(size_t)i] != 1 ? 1 : 0;
    std::fprintf(f, "%ld,%d,%d,%d,%.10g\n", frame_ids[(size_t)i], fr.status[(size_t)i], fr.corners[(size_t)i], fr.behind[(size_t)i], first[(size_t)i]);
  }
  std::fclose(f);
  auto reach = [&](int n) { return n ? std::to_string(n) : "more than " + std::to_string(r.order.size()); };
  std::printf("selected views: %zu of %d usable frames (%d shared columns); %s reach 90 %%, %s reach 99 %% of the attainable information, log-determinant gain %.6g\n",
              r.order.size(), usable, sel.Dim(), reach(n90).c_str(), reach(n99).c_str(), r.total);
  if (held_ids.empty()) return true;
  // which new view adds most: the held-out frames, at their refitted poses, as candidates against all calibrated frames
  const int H = (int)held_ids.size();
  std::vector<int> tile_frame(held.tile_frame);
  for (int& t : tile_frame) t += N;
  std::vector<double> poses((size_t)(N + H) * 7);
  for (int i = 0; i < N; ++i) { const vic::VicalibFrame fi = cal.GetFrame((size_t)i); std::copy(fi.t_wp_.data(), fi.t_wp_.data() + 7, &poses[(size_t)i * 7]); }
  if (held.T_wk.size() != (size_t)H * 7) { *err = "the held-out frames have no refitted poses"; return false; }
  std::copy(held.T_wk.begin(), held.T_wk.end(), poses.begin() + (size_t)N * 7);
  vic::Selector both(cal);
  both.SetPoses(poses.data(), N + H);
  both.AddTiles((int)tile_frame.size(), tile_frame.data(), held.tile_cam.data(), held.tile_off.data(), held.points.data(), (int)(held.points.size() / 3), held.point_id.data());
  std::vector<int> all(N);
  for (int i = 0; i < N; ++i) all[(size_t)i] = i;
  both.Run(1, all, o.prior);
  const std::vector<double> hfirst = both.LastGains();
  const vic::Selection hr = both.Run(H, all, o.prior);
  const vic::SelectionFrames hfr = both.Frames();
  std::vector<int> rank((size_t)H, 0);
  for (size_t k = 0; k < hr.order.size(); ++k) if (hr.order[k] >= N) rank[(size_t)(hr.order[k] - N)] = (int)k + 1;
  f = std::fopen((o.dir + "/select_holdout.csv").c_str(), "w");
  if (!f) { *err = "cannot write into " + o.dir; return false; }
  std::fprintf(f, "frame,holdout_status,status,corners,behind,first_round_gain,rank\n");
  for (int i = 0; i < H; ++i)
    std::fprintf(f, "%ld,%d,%d,%d,%d,%.10g,%d\n", held_ids[(size_t)i], held.status[(size_t)i], hfr.status[(size_t)(N + i)], hfr.corners[(size_t)(N + i)], hfr.behind[(size_t)(N + i)],
                 hfirst[(size_t)(N + i)], rank[(size_t)i]);
  std::fclose(f);
  return true;
}

int main(int argc, char** argv) {
  DefineFlags();
  std::string err;
  if (!ParseFlags(argc, argv, &err)) {
    if (err == "help") return Usage(0);
    std::fprintf(stderr, "ERROR: %s\n", err.c_str());
    return 1;
  }
  int report_bx = 16, report_by = 12;
  if (!ParseBins(FlagString("report_bins"), &report_bx, &report_by)) {
    std::fprintf(stderr, "ERROR: illegal value '%s' specified for flag 'report_bins': expected WIDTHxHEIGHT with both between 1 and 32\n", FlagString("report_bins").c_str());
    return 1;
  }
  const bool want_report = !FlagString("report_dir").empty() || FlagInt("report_worst") > 0;
  int holdout_every = 0;
  if (!ParseHoldoutEvery(FlagString("holdout_every"), &holdout_every)) {
    std::fprintf(stderr, "ERROR: illegal value '%s' specified for flag 'holdout_every': expected 0 (off) or N >= 2 (N = 1 would leave no frame to calibrate from)\n", FlagString("holdout_every").c_str());
    return 1;
  }
  if (FlagBool("seed_focal")) {
    if (!FlagString("model_files").empty()) { std::fprintf(stderr, "ERROR: -seed_focal and -model_files exclude each other: a model file brings its own focal length\n"); return 1; }
    if (!(FlagDouble("seed_focal_fit_px") >= 0.0)) { std::fprintf(stderr, "ERROR: illegal value for flag 'seed_focal_fit_px': expected at least 0\n"); return 1; }
  }
  if (FlagBool("seed_imu")) {
    if (FlagString("imu").empty()) { std::fprintf(stderr, "ERROR: -seed_imu needs -imu: there is no log to seed from\n"); return 1; }
    if (!FlagBool("calibrate_imu")) { std::fprintf(stderr, "ERROR: -seed_imu and -nocalibrate_imu exclude each other: nothing would use the seed\n"); return 1; }
    if (FlagBool("has_initial_guess")) { std::fprintf(stderr, "ERROR: -seed_imu and -has_initial_guess exclude each other: the guess is the start\n"); return 1; }
    if (!(FlagDouble("seed_imu_range") > 0.0) || !std::isfinite(FlagDouble("seed_imu_range"))) { std::fprintf(stderr, "ERROR: illegal value for flag 'seed_imu_range': expected more than 0\n"); return 1; }
    if (!std::isfinite(FlagDouble("seed_imu_step"))) { std::fprintf(stderr, "ERROR: illegal value for flag 'seed_imu_step': expected a number (0: the median sample interval)\n"); return 1; }
    if (!(FlagDouble("seed_imu_max_gap") > 0.0)) { std::fprintf(stderr, "ERROR: illegal value for flag 'seed_imu_max_gap': expected more than 0\n"); return 1; }
    if (FlagInt("seed_imu_min_intervals") < 1) { std::fprintf(stderr, "ERROR: illegal value for flag 'seed_imu_min_intervals': expected at least 1\n"); return 1; }
  }
  UncertaintyOptions uncertainty;
  if (!UncertaintyFlags(&uncertainty, &err)) { std::fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
  StereoUncertaintyOptions stereo_uncertainty;
  if (!StereoUncertaintyFlags(&stereo_uncertainty, &err)) { std::fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
  SelectOptions select;
  if (!SelectFlags(&select, &err)) { std::fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
  // ---- -compare_models a.xml,b.xml: file against file, nothing is calibrated; -compare_to b.xml: read now, compared behind the results
  CompareOptions compare;
  std::vector<vic::CameraAndPose> compare_b;
  if (!FlagString("compare_models").empty() || !FlagString("compare_to").empty()) {
    if (!FlagString("compare_models").empty() && !FlagString("compare_to").empty()) { std::fprintf(stderr, "ERROR: -compare_models and -compare_to exclude each other\n"); return 1; }
    if (!CompareFlags(&compare, &err)) { std::fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
  }
  // ---- -convert_models in.xml -convert_to m[,m...]: file to file, nothing is calibrated; -convert_to alone: the result is converted behind it
  ConvertOptions convert;
  const bool converting = !FlagString("convert_models").empty() || !FlagString("convert_to").empty();
  if (converting) {
    if (!FlagString("compare_models").empty() || !FlagString("compare_to").empty()) { std::fprintf(stderr, "ERROR: -convert_models / -convert_to and -compare_models / -compare_to exclude each other\n"); return 1; }
    if (!ConvertFlags(&convert, &err)) { std::fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
    if (!FlagString("compare_dir").empty()) {
      if (!CompareFlags(&compare, &err)) { std::fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
      compare.identity = true; compare.gx = convert.gx; compare.gy = convert.gy;      // (the conversion's own lattice; -compare_grid is not read)
    }
  }
  // ---- -register_models rig.xml -register_depth ...: file to file, nothing is calibrated; -register_depth alone: the result registers behind it
  RegisterOptions reg;
  if (!RegisterFlags(&reg, &err)) { std::fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
  if (reg.on && (!FlagString("compare_models").empty() || !FlagString("convert_models").empty())) {
    std::fprintf(stderr, "ERROR: -register_models / -register_depth and -compare_models / -convert_models exclude each other\n"); return 1;
  }
  // ---- -depthcal_models rig.xml -depthcal_poses ... / -depthcal_apply file: file to file, nothing is calibrated; -depthcal_depth alone: behind the result
  DepthCalCli depthcal;
  if (!DepthCalFlags(&depthcal, &err)) { std::fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
  if (depthcal.on && (!FlagString("compare_models").empty() || !FlagString("convert_models").empty() || !FlagString("register_models").empty())) {
    std::fprintf(stderr, "ERROR: -depthcal_models / -depthcal_depth / -depthcal_apply and -compare_models / -convert_models / -register_models exclude each other\n"); return 1;
  }
  // ---- -allan_imu csv://log -allan_dir dir: the IMU's noise from a static log, nothing is calibrated
  AllanCli allan;
  if (!AllanFlags(&allan, &err)) { std::fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
  if (allan.on) {
    const int rc = AllanImu(allan, (int)FlagInt("device"), &err);
    if (rc != 0) std::fprintf(stderr, "%s %s\n", rc == 3 ? "F" : "E IMU noise characterisation failed:", err.c_str());
    return rc;
  }
  if (depthcal.apply) {
    const int rc = DepthCalApply(depthcal, (int)FlagInt("device"), &err);
    if (rc != 0) std::fprintf(stderr, "%s %s\n", rc == 3 ? "F" : "E depth correction failed:", err.c_str());
    return rc;
  }
  if (!depthcal.models.empty()) {
    std::vector<vic::CameraAndPose> a;
    std::vector<std::array<double, 7>> poses;
    if (!ReadRigFile(depthcal.models, &a, &err) || !ReadPoseFile(depthcal.poses, &poses, &err)) { std::fprintf(stderr, "F %s\n", err.c_str()); return 1; }
    const int rc = DepthCalFit(a, poses, "-depthcal_poses", depthcal, (int)FlagInt("device"), &err);
    if (rc != 0) std::fprintf(stderr, "%s %s\n", rc == 3 ? "F" : "E depth calibration failed:", err.c_str());
    return rc;
  }
  if (!FlagString("register_models").empty()) {
    std::vector<vic::CameraAndPose> a;
    if (!ReadRigFile(FlagString("register_models"), &a, &err)) { std::fprintf(stderr, "F %s\n", err.c_str()); return 1; }
    const int rc = RegisterRig(a, reg, (int)FlagInt("device"), &err);
    if (rc != 0) std::fprintf(stderr, "%s %s\n", rc == 3 ? "F" : "E registration failed:", err.c_str());
    return rc;
  }
  if (!FlagString("convert_models").empty()) {
    std::vector<vic::CameraAndPose> a;
    if (!ReadRigFile(FlagString("convert_models"), &a, &err)) { std::fprintf(stderr, "F %s\n", err.c_str()); return 1; }
    if (!ConvertibleRig(a, convert, &err)) { std::fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
    const int rc = ConvertRig(FlagString("convert_models"), a, convert, compare.identity ? &compare : nullptr, (int)FlagInt("device"), &err);
    if (rc != 0) std::fprintf(stderr, "%s %s\n", rc == 3 ? "F" : "E conversion failed:", err.c_str());
    return rc;
  }
  if (!FlagString("compare_models").empty()) {
    const std::string& both = FlagString("compare_models");
    const size_t comma = both.find(',');
    if (comma == std::string::npos || comma == 0 || comma + 1 >= both.size() || both.find(',', comma + 1) != std::string::npos) {
      std::fprintf(stderr, "ERROR: illegal value '%s' specified for flag 'compare_models': expected a.xml,b.xml\n", both.c_str()); return 1;
    }
    std::vector<vic::CameraAndPose> a;
    if (!ReadRigFile(both.substr(0, comma), &a, &err) || !ReadRigFile(both.substr(comma + 1), &compare_b, &err)) { std::fprintf(stderr, "F %s\n", err.c_str()); return 1; }
    const int rc = CompareRigs(a, compare_b, compare, (int)FlagInt("device"), &err);
    if (rc != 0) std::fprintf(stderr, "%s %s\n", rc == 3 ? "F" : "E comparison failed:", err.c_str());
    return rc;
  }
  if (!FlagString("compare_to").empty() && !ReadRigFile(FlagString("compare_to"), &compare_b, &err)) { std::fprintf(stderr, "F %s\n", err.c_str()); return 1; }
  if (FlagString("cam").empty()) { std::fprintf(stderr, "F No camera URI given\n"); return 1; }      // vicalib-engine.cc:445
  // ---- grid (vicalib-engine.cc:449-464): the detections already carry X,Y,Z; the preset only bounds the dot ids ----
  int grid_w = (int)FlagInt("grid_width"), grid_h = (int)FlagInt("grid_height");
  const std::string preset = FlagString("grid_preset");
  if (!preset.empty()) {
    if (preset == "small" || preset == "0" || preset == "letter") { grid_w = 19; grid_h = 10; }
    else if (preset == "large" || preset == "1") { grid_w = 36; grid_h = 25; }
    else if (preset == "medium") { grid_w = 1 << 15; grid_h = 1; }     // size not recorded in the reference tree: no bound on dot ids
    else { std::fprintf(stderr, "F Unknown grid preset %s\n", preset.c_str()); return 1; }
  }
  // ---- sensors ------------------------------------------------------------------------------------------------------
  const std::vector<std::string> cam_files = Split(StripScheme(FlagString("cam")), ',');
  std::vector<Channel> channels(cam_files.size());
  const bool from_images = FlagString("cam").compare(0, 7, "file://") == 0;      // HAL's FileReader scheme (main.cc:11)
  int img_w = 0, img_h = 0;
  if (from_images) {
    // the target (vicalib-engine.cc:453-465): its pattern from a file, or generated from -grid_height / -grid_width / -grid_seed
    TargetSpec tg;
    tg.rows = grid_h; tg.cols = grid_w; tg.spacing = FlagDouble("grid_spacing");
    if (!FlagString("grid_pattern_file").empty()) {
      std::ifstream pf(FlagString("grid_pattern_file"));
      if (!pf) { std::fprintf(stderr, "F cannot open grid pattern file %s\n", FlagString("grid_pattern_file").c_str()); return 1; }
      std::string line; std::vector<double> v; tg.rows = 0; tg.cols = 0;
      while (std::getline(pf, line)) {
        if (line.empty() || line[0] == '#') continue;
        if (!ParseNumbers(line, &v) || v.empty()) continue;
        if (tg.cols && (int)v.size() != tg.cols) { std::fprintf(stderr, "F grid pattern file: rows of different length\n"); return 1; }
        tg.cols = (int)v.size(); ++tg.rows;
        for (double x : v) tg.pattern.push_back(x != 0.0 ? 1 : 0);
      }
      if (tg.rows < 2 || tg.cols < 2) { std::fprintf(stderr, "F grid pattern file holds no pattern\n"); return 1; }
      grid_w = tg.cols; grid_h = tg.rows;
    } else if (!preset.empty()) {
      std::fprintf(stderr, "F -grid_preset %s with image input: the presets' large / small patterns live in Calibu, which is not part of the reference tree -- "
                           "pass the printed target's pattern with -grid_pattern_file (or generate a target with -grid_height / -grid_width / -grid_seed)\n", preset.c_str());
      return 1;
    } else {
      tg.pattern.resize((size_t)tg.rows * tg.cols);
      vc_target_make_pattern(tg.rows, tg.cols, (unsigned)FlagInt("grid_seed"), tg.pattern.data());
    }
    for (size_t c = 0; c < cam_files.size(); ++c) {
      int w = 0, h = 0;
      if (!ReadImages(cam_files[c], tg, (int)FlagInt("device"), &channels[c], &w, &h, &err)) { std::fprintf(stderr, "F %s\n", err.c_str()); return err.find("HIP device") != std::string::npos ? 3 : 1; }
      img_w = std::max(img_w, w); img_h = std::max(img_h, h);
    }
  } else
  for (size_t c = 0; c < cam_files.size(); ++c)
    if (!ReadDetections(cam_files[c], &channels[c], &err)) { std::fprintf(stderr, "F %s\n", err.c_str()); return 1; }
  const size_t n_cam = channels.size();
  int rectify_a = 0, rectify_b = 1;
  if (!FlagString("rectify_dir").empty()) {
    if (n_cam < 2) { std::fprintf(stderr, "E -rectify_dir needs two cameras (-cam has %zu)\n", n_cam); return 1; }
    if (!ParseRectifyCams(FlagString("rectify_cams"), n_cam, &rectify_a, &rectify_b)) {
      std::fprintf(stderr, "E illegal value '%s' specified for flag 'rectify_cams': expected a,b, two different cameras below %zu\n", FlagString("rectify_cams").c_str(), n_cam);
      return 1;
    }
    if (!(FlagDouble("rectify_alpha") >= 0.0 && FlagDouble("rectify_alpha") <= 1.0)) { std::fprintf(stderr, "E illegal value for flag 'rectify_alpha': expected 0 ... 1\n"); return 1; }
  }
  ImuData imu;
  const bool have_imu = !FlagString("imu").empty();
  if (have_imu && !ReadImu(StripScheme(FlagString("imu")), FlagBool("use_system_time"), &imu, &err)) { std::fprintf(stderr, "F %s\n", err.c_str()); return 1; }
  bool calibrate_imu = FlagBool("calibrate_imu");
  if (calibrate_imu && !have_imu) { std::fprintf(stderr, "W -calibrate_imu without -imu: calibrating the cameras only\n"); calibrate_imu = false; }

  // ---- start cameras (vicalib-engine.cc:162-257) -------------------------------------------------------------------
  std::vector<std::string> models = Split(FlagString("models"), ','), model_files = Split(FlagString("model_files"), ',');
  if (model_files.empty() && models.size() < n_cam) {
    std::fprintf(stderr, "I Only %zu models declared; need one for all the %zu channels; assuming poly3\n", models.size(), n_cam);
    models.resize(n_cam, "poly3");
  }
  std::vector<vic::CameraAndPose> input_cameras;
  const int W = img_w > 0 ? img_w : (int)FlagInt("image_width"), H = img_h > 0 ? img_h : (int)FlagInt("image_height");      // (images carry their size)
  if (!model_files.empty()) {
    for (const std::string& mf : model_files) {
      vic::CameraAndPose cam;
      if (!ReadModelFile(mf, &cam, &err)) { std::fprintf(stderr, "F %s\n", err.c_str()); return 1; }
      if (cam.width == 0) { cam.width = W; cam.height = H; }
      input_cameras.push_back(cam);
    }
  } else {
    for (const std::string& type : models) {
      vic::CameraAndPose cam;
      cam.model = ModelId(type);
      if (cam.model < 0) { std::fprintf(stderr, "F camera model '%s' is not supported by this build (fov, poly2, poly3, rational6, kb4, linear)\n", type.c_str()); return 1; }
      cam.width = W; cam.height = H;
      cam.params = {300, 300, W / 2.0, H / 2.0};
      if (cam.model == VC_MODEL_FOV) cam.params.push_back(0.2);
      else cam.params.resize(cam.model == VC_MODEL_POLY2 ? 6 : cam.model == VC_MODEL_POLY3 ? 7 : cam.model == VC_MODEL_KB4 ? 8 : cam.model == VC_MODEL_RATIONAL6 ? 10 : 4, 0.0);
      input_cameras.push_back(cam);
    }
  }
  if (input_cameras.size() < n_cam) { std::fprintf(stderr, "F %zu camera models for %zu channels\n", input_cameras.size(), n_cam); return 1; }
  input_cameras.resize(n_cam);
  if (converting && !ConvertibleRig(input_cameras, convert, &err)) { std::fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }      // before any solve
  if (!uncertainty.dir.empty()) {
    if (!FlagBool("calibrate_intrinsics")) { std::fprintf(stderr, "F -uncertainty_dir needs -calibrate_intrinsics: fixed intrinsics have no covariance\n"); return 1; }
    for (size_t c = 0; c < input_cameras.size(); ++c)
      if (uncertainty.gx > input_cameras[c].width || uncertainty.gy > input_cameras[c].height) { std::fprintf(stderr, "F camera %zu: -uncertainty_grid exceeds the image\n", c); return 1; }
  }
  if (!stereo_uncertainty.dir.empty()) {
    const StereoUncertaintyOptions& su = stereo_uncertainty;
    if ((size_t)su.a >= n_cam || (size_t)su.b >= n_cam) { std::fprintf(stderr, "E illegal value '%s' specified for flag 'stereo_uncertainty_cams': expected two cameras below %zu\n", FlagString("stereo_uncertainty_cams").c_str(), n_cam); return 1; }
    if (!FlagBool("calibrate_intrinsics")) { std::fprintf(stderr, "F -stereo_uncertainty_dir needs -calibrate_intrinsics: fixed intrinsics have no covariance\n"); return 1; }
    if (su.gx > input_cameras[su.a].width || su.gy > input_cameras[su.a].height) { std::fprintf(stderr, "F -stereo_uncertainty_grid exceeds the image of camera %d\n", su.a); return 1; }
  }
  if (!compare_b.empty() && !ComparableRigs(input_cameras, compare_b, compare, &err)) { std::fprintf(stderr, "F -compare_to: %s\n", err.c_str()); return 1; }      // before any solve

  // ---- frames: union of the frame ids, -frame_skip, -num_vicalib_frames (vicalib-engine.cc:540-590) ---------------------
  std::set<long> ids;
  for (const Channel& ch : channels) for (const Detection& d : ch.det) ids.insert(d.frame);
  std::vector<long> frame_ids;
  {
    const long skip = FlagInt("frame_skip"), limit = FlagInt("num_vicalib_frames");
    long k = 0;
    for (long id : ids) {
      if (skip > 0 && (k++ % (skip + 1)) != 0) continue;
      if (limit >= 0 && (long)frame_ids.size() >= limit) break;
      frame_ids.push_back(id);
    }
  }
  if (frame_ids.empty()) { std::fprintf(stderr, "F no usable frames in the detections\n"); return 1; }
  // ---- -holdout_every N: every Nth surviving frame is not a frame of the problem (vc_holdout_select.hpp); it is scored afterwards.  The IMU
  // stream is unchanged: the blocks simply span the gaps
  std::vector<long> held_ids;
  if (holdout_every > 0) {
    if (!vc::holdout_every_ok((long long)frame_ids.size(), holdout_every)) {
      std::fprintf(stderr, "ERROR: illegal value '%d' specified for flag 'holdout_every': it leaves fewer than 2 of the %zu frames to calibrate from\n", holdout_every, frame_ids.size());
      return 1;
    }
    std::vector<long> fit;
    for (size_t i = 0; i < frame_ids.size(); ++i) (vc::holdout_is_held((long long)i, holdout_every) ? held_ids : fit).push_back(frame_ids[i]);
    frame_ids.swap(fit);
  }

  // ---- -seed_focal: fx = fy of every camera from the homographies of its views in the frames that will be calibrated (held-out frames are
  // not among them), one batch on -device; the one result serves every rank
  if (FlagBool("seed_focal")) {
    const std::set<long> fit_ids(frame_ids.begin(), frame_ids.end());
    std::vector<int> view_cam, view_off(1, 0);
    std::vector<double> pp, radius, pw, pc;
    const double frac = FlagDouble("seed_focal_radius");
    for (size_t c = 0; c < n_cam; ++c) {
      const double w = input_cameras[c].width, h = input_cameras[c].height;
      pp.insert(pp.end(), {w / 2.0, h / 2.0});
      radius.push_back(frac > 0.0 ? frac * 0.5 * std::sqrt(w * w + h * h) : 0.0);
      std::map<long, std::vector<const Detection*>> per_frame;
      for (const Detection& d : channels[c].det)
        if (fit_ids.count(d.frame) && d.dot < grid_w * grid_h) per_frame[d.frame].push_back(&d);
      for (const auto& kv : per_frame) {
        for (const Detection* d : kv.second) { pw.insert(pw.end(), {d->X, d->Y, d->Z}); pc.insert(pc.end(), {d->u, d->v}); }
        view_cam.push_back((int)c); view_off.push_back((int)(pc.size() / 2));
      }
    }
    vic::SeedFocalResult sf;
    try { sf = vic::SeedFocalBatch((int)FlagInt("device"), view_cam, pp, radius, view_off, pw, pc, 4, FlagDouble("seed_focal_fit_px")); }
    catch (const std::exception& e) { std::fprintf(stderr, "F -seed_focal: %s (device %d)\n", e.what(), (int)FlagInt("device")); return 3; }
    for (size_t c = 0; c < n_cam; ++c) {
      int total = 0;
      std::vector<double> fv;
      for (size_t v = 0; v < view_cam.size(); ++v) {
        if (view_cam[v] != (int)c) continue;
        ++total;
        if (sf.view_status[v] == 0 && std::isfinite(sf.view_f[v])) fv.push_back(sf.view_f[v]);
      }
      if (sf.cam_status[c] == 0) {
        input_cameras[c].params[0] = input_cameras[c].params[1] = sf.cam_f[c];
        std::sort(fv.begin(), fv.end());
        if (fv.empty()) std::fprintf(stderr, "I camera %zu: focal length seed %.2f px from %d of %d views\n", c, sf.cam_f[c], sf.cam_views[c], total);
        else std::fprintf(stderr, "I camera %zu: focal length seed %.2f px from %d of %d views (single views: %.2f .. %.2f px, median %.2f, %zu of them tilted enough)\n",
                          c, sf.cam_f[c], sf.cam_views[c], total, fv.front(), fv.back(), fv[fv.size() / 2], fv.size());
      } else {
        const char* why = sf.cam_status[c] == 1 ? "no usable view" : sf.cam_status[c] == 2 ? "the target was never tilted against the image plane" : "the views give no positive focal length";
        std::fprintf(stderr, "W camera %zu: no focal length seed (%s, %d of %d views usable); keeping fx = fy = %g\n", c, why, sf.cam_views[c], total, input_cameras[c].params[0]);
      }
    }
  }

  const bool guess = FlagBool("has_initial_guess");
  // initial time offset (vicalib-task.cc:638-662): with system time the clocks are already aligned
  double image_time_offset = 0.0;
  {
    double t0f = (double)frame_ids[0] / FlagDouble("frame_rate");
    for (const Channel& ch : channels) { auto it = ch.frame_time.find(frame_ids[0]); if (it != ch.frame_time.end()) { t0f = it->second; break; } }
    if (calibrate_imu && FlagBool("find_time_offset") && !FlagBool("use_system_time") && !imu.time.empty()) image_time_offset = imu.time[0] - t0f;
  }

  // ---- -seed_imu: R_ck of camera 0, the time offset, the gyro bias and gravity from the rates of camera 0's PnP rotations against the gyro's,
  // one batch on -device before any calibrator exists; the one result serves every rank.  Any status but 0: a W line, today's start.
  vic::SeedImuResult imu_seed;
  if (FlagBool("seed_imu")) {
    const vic::CameraAndPose& cam0 = input_cameras[0];
    std::map<long, std::vector<const Detection*>> per_frame;
    for (const Detection& d : channels[0].det)
      if (d.dot < grid_w * grid_h) per_frame[d.frame].push_back(&d);
    std::vector<int> view_model, view_off(1, 0), view_frame;
    std::vector<double> view_K, pw, pc, frame_t(frame_ids.size()), frame_q(4 * frame_ids.size(), 0.0);
    std::vector<unsigned char> frame_ok(frame_ids.size(), 0);
    for (size_t k = 0; k < frame_ids.size(); ++k) {
      const long id = frame_ids[k];
      double t = (double)id / FlagDouble("frame_rate");
      for (const Channel& ch : channels) { auto it = ch.frame_time.find(id); if (it != ch.frame_time.end()) { t = it->second; break; } }
      frame_t[k] = t + image_time_offset;                                 // the time the calibrators get
      frame_q[4 * k + 3] = 1.0;
      auto it = per_frame.find(id);
      if (it == per_frame.end() || it->second.size() < 4) continue;
      for (const Detection* d : it->second) { pw.insert(pw.end(), {d->X, d->Y, d->Z}); pc.insert(pc.end(), {d->u, d->v}); }
      view_model.push_back(cam0.model); view_off.push_back((int)(pc.size() / 2)); view_frame.push_back((int)k);
      for (size_t j = 0; j < 10; ++j) view_K.push_back(j < cam0.params.size() ? cam0.params[j] : 0.0);
    }
    const int nv = (int)view_frame.size();
    std::vector<double> T_cw(7 * (size_t)nv + 7, 0.0), rms((size_t)nv + 1, 0.0);
    std::vector<int> n_in((size_t)nv + 1, 0), pnp_status((size_t)nv + 1, -1);
    int rc = nv > 0 ? vc_pnp_planar_batch((int)FlagInt("device"), nv, view_model.data(), view_K.data(), view_off.data(), pw.data(), pc.data(), (int)FlagInt("pnp_ransac_its"),
                                          FlagDouble("pnp_ransac_tol"), T_cw.data(), rms.data(), n_in.data(), nullptr, pnp_status.data())
                    : VC_OK;
    if (rc == VC_ERR_NO_DEVICE) { std::fprintf(stderr, "F -seed_imu: no HIP device %d\n", (int)FlagInt("device")); return 3; }
    int n_ok = 0;
    for (int v = 0; v < nv && rc == VC_OK; ++v) {
      if (pnp_status[v] != 0) continue;
      const size_t k = (size_t)view_frame[v];
      for (int j = 0; j < 3; ++j) frame_q[4 * k + j] = -T_cw[7 * (size_t)v + j];      // R_wc = R_cw^T
      frame_q[4 * k + 3] = T_cw[7 * (size_t)v + 3];
      frame_ok[k] = 1; ++n_ok;
    }
    if (rc == VC_OK) {
      try {
        imu_seed = vic::SeedImu((int)FlagInt("device"), frame_t, frame_q, frame_ok, imu.time, imu.gyro, imu.accel, FlagDouble("seed_imu_range"), FlagDouble("seed_imu_step"), 8,
                                FlagDouble("seed_imu_max_gap"), (int)FlagInt("seed_imu_min_intervals"));
      } catch (const std::exception& e) {
        if (std::string(e.what()).find("status -1)") != std::string::npos) { std::fprintf(stderr, "F -seed_imu: no HIP device %d\n", (int)FlagInt("device")); return 3; }
        std::fprintf(stderr, "W -seed_imu: %s; starting without the seed\n", e.what());
      }
    } else std::fprintf(stderr, "W -seed_imu: the pose batch of camera 0 failed (status %d); starting without the seed\n", rc);
    if (imu_seed.status == 0) {
      const double* R = imu_seed.R_ck;
      const vic::Se3 old0 = input_cameras[0].T_ck;
      double q[4];
      RotationToQuat(R, q);
      for (int j = 0; j < 4; ++j) input_cameras[0].T_ck.v[j] = q[j];                    // the translation stays
      for (size_t c = 1; c < n_cam; ++c) input_cameras[c].T_ck = Se3Mul(Se3Mul(input_cameras[c].T_ck, Se3Inverse(old0)), input_cameras[0].T_ck);      // the rig's relative poses stay
      const double angle = 2.0 * std::atan2(std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), std::fabs(q[3])) * 180.0 / M_PI;
      std::fprintf(stderr, "I -seed_imu: time offset %.6f ms, R_ck [qx qy qz qw] %.9f %.9f %.9f %.9f (%.3f degrees from identity), gyro bias %.6g %.6g %.6g, "
                           "gravity %.6g %.6g, rms / signal %.4f, %d intervals (%d of %zu frames with a rotation)\n",
                   1e3 * imu_seed.time_offset, q[0], q[1], q[2], q[3], angle, imu_seed.gyro_bias[0], imu_seed.gyro_bias[1], imu_seed.gyro_bias[2], imu_seed.g_dir[0],
                   imu_seed.g_dir[1], imu_seed.rms / imu_seed.signal, imu_seed.count, n_ok, frame_ids.size());
      if (imu_seed.rms > 0.5 * imu_seed.signal)
        std::fprintf(stderr, "W -seed_imu: the camera's rates and the gyro's explain each other badly (rms / signal %.2f above 0.5): too little rotation about two axes?\n", imu_seed.rms / imu_seed.signal);
    } else if (imu_seed.status > 0) {
      const char* why = imu_seed.status == 1 ? "too few frame intervals with a rate inside the log" : imu_seed.status == 2 ? "the best offset lies on the edge of -seed_imu_range" : "a result is not finite";
      std::fprintf(stderr, "W -seed_imu: no seed (%s; %d of %zu frames with a rotation); starting without it\n", why, n_ok, frame_ids.size());
    }
  }

  // ---- one calibrator per GPU; frames sharded contiguously, the library's own RCCL communicator does the per-iteration
  // all-reduces (-gpus 1: plain single-device run, no communicator) -----------------------------------------------------
  const int n_gpus = std::max(1, (int)FlagInt("gpus"));
  if ((size_t)n_gpus * 2 > frame_ids.size()) { std::fprintf(stderr, "F -gpus %d needs at least %d frames\n", n_gpus, 2 * n_gpus); return 1; }
  std::vector<std::unique_ptr<vic::ViCalibrator>> cals((size_t)n_gpus);
  for (int r = 0; r < n_gpus; ++r) {
    try { cals[r].reset(new vic::ViCalibrator((int)FlagInt("device") + r)); }
    catch (const std::exception& e) { std::fprintf(stderr, "F %s (device %d)\n", e.what(), (int)FlagInt("device") + r); return 3; }
  }
  long n_obs = 0; int seeded = 0;
  std::vector<std::vector<const Detection*>> rank_corners((size_t)n_gpus);      // (report) the detection behind every corner, in the order it was added
  for (int r = 0; r < n_gpus; ++r) {
    vic::ViCalibrator& cal = *cals[r];
    cal.SetSigmas(FlagDouble("gyro_sigma"), FlagDouble("accel_sigma"));                     // vicalib-engine.cc:301-303
    const double zeros[6] = {0, 0, 0, 0, 0, 0}, ones[6] = {1, 1, 1, 1, 1, 1};
    cal.SetBiases(zeros); cal.SetScaleFactor(ones);
    cal.FixCameraIntrinsics(!FlagBool("calibrate_intrinsics"));                            // vicalib-task.cc:128
    for (const vic::CameraAndPose& c : input_cameras)
      if (cal.AddCamera(c) < 0) { std::fprintf(stderr, "F AddCamera failed (model %s, %zu parameters)\n", ModelName(c.model), c.params.size()); return 1; }
    // every shard gets the whole IMU stream: its last block reaches into the next shard's first frame
    if (have_imu && !imu.time.empty() && cal.AddImuMeasurements((int)imu.time.size(), imu.gyro.data(), imu.accel.data(), imu.time.data()) != VC_OK) {
      std::fprintf(stderr, "F IMU measurements rejected\n"); return 1;
    }
    const size_t lo = frame_ids.size() * (size_t)r / (size_t)n_gpus, hi = frame_ids.size() * (size_t)(r + 1) / (size_t)n_gpus;
    std::map<long, int> frame_index;
    vic::Se3 placeholder; placeholder.v = {{0, 0, 0, 1, 0, 0, 1000}};                       // vicalib-task.cc:241-244
    for (size_t k = lo; k < hi; ++k) {
      const long id = frame_ids[k];
      double t = (double)id / FlagDouble("frame_rate");
      for (const Channel& ch : channels) { auto it = ch.frame_time.find(id); if (it != ch.frame_time.end()) { t = it->second; break; } }
      frame_index[id] = cal.AddFrame(placeholder, t + image_time_offset);
    }
    std::vector<double> pw, pc;
    for (size_t c = 0; c < n_cam; ++c) {
      std::map<int, std::vector<const Detection*>> per_frame;
      for (const Detection& d : channels[c].det) {
        auto it = frame_index.find(d.frame);
        if (it == frame_index.end()) continue;
        if (d.dot >= grid_w * grid_h) continue;                 // outside the declared grid (vicalib-task.cc:353-354)
        per_frame[it->second].push_back(&d);
      }
      for (const auto& kv : per_frame) {
        pw.clear(); pc.clear();
        for (const Detection* d : kv.second) {
          pw.insert(pw.end(), {d->X, d->Y, d->Z}); pc.insert(pc.end(), {d->u, d->v});
          if (FlagBool("output_conics")) std::printf("%ld,%d,%.10g,%.10g,%.10g,%.10g,%.10g\n", d->frame, d->dot, d->u, d->v, d->X, d->Y, d->Z);
        }
        cal.AddObservations(kv.first, c, (int)kv.second.size(), pw.data(), pc.data());
        if (want_report) rank_corners[r].insert(rank_corners[r].end(), kv.second.begin(), kv.second.end());
        n_obs += (long)kv.second.size();
      }
    }
    if (imu_seed.status == 0) {                                                            // -seed_imu: the same start on every rank
      const double b[6] = {imu_seed.gyro_bias[0], imu_seed.gyro_bias[1], imu_seed.gyro_bias[2], 0, 0, 0};
      cal.SetTimeOffset(imu_seed.time_offset); cal.SetBiases(b);
      if (vc_set_gravity(cal.handle(), imu_seed.g_dir) != VC_OK) { std::fprintf(stderr, "F the gravity seed was rejected\n"); return 1; }
    }
    cal.SetPnPRansac((int)FlagInt("pnp_ransac_its"), FlagDouble("pnp_ransac_tol"));
    cal.SetPnPDevice(FlagBool("pnp_device"));
    seeded += cal.InitFramePosesPnP();
    // ---- VicalibTask::Start(has_initial_guess) (vicalib-task.cc:226-234) + flags read inside the calibrator ---------
    cal.SetOptimizationFlags(guess, guess && calibrate_imu, !guess, FlagBool("find_time_offset"));
    cal.SetFunctionTolerance(FlagDouble("function_tolerance"));
    cal.SetMaxIters((int)FlagInt("max_iters"));
    cal.SetCalibrateImu(calibrate_imu);
    cal.SetRemoveOutliers(FlagBool("remove_outliers"), FlagDouble("outlier_threshold"));
  }
  std::fprintf(stderr, "I %zu cameras, %zu frames on %d GPU(s) (%d with a PnP seed), %ld corner observations, %zu IMU samples\n", n_cam, frame_ids.size(), n_gpus, seeded, n_obs, imu.time.size());
  if (n_gpus > 1) {
    char id[128];
    if (vc_rccl_unique_id(id) != VC_OK) { std::fprintf(stderr, "F RCCL is not available (librccl.so)\n"); return 3; }
    std::vector<int> rc((size_t)n_gpus, 0);
    std::vector<std::thread> th;
    for (int r = 0; r < n_gpus; ++r) th.emplace_back([&, r] { rc[r] = vc_set_shard_rccl(cals[r]->handle(), r, n_gpus, id); });   // ncclCommInitRank: collective
    for (std::thread& t : th) t.join();
    for (int r = 0; r < n_gpus; ++r) if (rc[r] != VC_OK) { std::fprintf(stderr, "F RCCL communicator setup failed on rank %d (%d)\n", r, rc[r]); return 3; }
  }
  vic::ViCalibrator& cal = *cals[0];              // shared parameters and statistics are identical on every rank
  const auto t0 = std::chrono::steady_clock::now();
  for (auto& c : cals) c->Start();
  unsigned last_iters = ~0u;
  auto any_running = [&] { for (auto& c : cals) if (c->IsRunning()) return true; return false; };
  while (any_running()) {                                         // vicalib-engine.cc:376-431, 30 ms
    const unsigned it = cal.GetNumIterations();
    if (it != last_iters) { std::fprintf(stderr, "I iteration %u  mse %.6g\n", it, cal.MeanSquaredError()); last_iters = it; }
    std::this_thread::sleep_for(std::chrono::milliseconds(30));
  }
  for (auto& c : cals) c->Stop();
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  // frames of all shards, in order
  std::vector<vic::VicalibFrame> all_frames;
  for (auto& c : cals) for (size_t i = 0; i < c->NumFrames(); ++i) all_frames.push_back(c->GetFrame(i));

  // ---- Finish + PrintResults (vicalibrator.h:536-544) ------------------------------------------------------------------
  const std::vector<double> rmse = cal.GetCameraProjRMSE();
  std::printf("------------------------------------------\n");
  for (size_t c = 0; c < n_cam; ++c) {
    const vic::CameraAndPose cam = cal.GetCamera(c);
    std::printf("Camera: %zu (%s)\n ", c, ModelName(input_cameras[c].model));
    for (double p : cam.params) std::printf(" %.10g", p);
    std::printf("\n  T_ck [qx qy qz qw tx ty tz]:");
    for (double p : cam.T_ck.v) std::printf(" %.10g", p);
    std::printf("\n  reprojection RMSE: %.6g px\n", rmse[c]);
  }
  if (calibrate_imu) {
    const auto b = cal.GetBiases(), s = cal.GetScaleFactor(); const auto g = cal.GetGravity();
    std::printf("IMU biases (gyro, accel): %.8g %.8g %.8g  %.8g %.8g %.8g\n", b[0], b[1], b[2], b[3], b[4], b[5]);
    std::printf("IMU scale factors:        %.8g %.8g %.8g  %.8g %.8g %.8g\n", s[0], s[1], s[2], s[3], s[4], s[5]);
    std::printf("gravity direction: %.8g %.8g   time offset: %.9g s\n", g[0], g[1], cal.time_offset());
  }
  std::printf("iterations: %u  mse: %.8g  solve time: %.3f s\n", cal.GetNumIterations(), cal.MeanSquaredError(), secs);
  if (FlagBool("print_covariance")) {       // GetSolutionCovariance + its log lines (vicalibrator.h:802-857, :1004-1013)
    std::vector<std::vector<double>> covs((size_t)n_gpus);
    std::vector<int> dims((size_t)n_gpus, 0);
    std::vector<std::thread> th;            // collective when the frames are sharded: every rank linearises
    for (int r = 0; r < n_gpus; ++r) th.emplace_back([&, r] { covs[r] = cals[r]->GetSolutionCovariance(&dims[r]); });
    for (auto& t : th) t.join();
    if (dims[0] > 0) {
      std::printf("Covariance calculated for blocks: %s\nSolution covariance:\n", cal.covariance_names().c_str());
      for (int i = 0; i < dims[0]; ++i) {
        for (int j = 0; j < dims[0]; ++j) std::printf(" %.6e", covs[0][(size_t)i * dims[0] + j]);
        std::printf("\n");
      }
    } else std::printf("Failed to compute covariance...\n");
  }

  // ---- residual report (-report_dir, -report_worst): per rank, rows concatenated in frame order, maps summed ----------------------------
  if (want_report) {
    struct ViewRow { long frame; int cam, count, removed; double rmse, max_err; int worst_dot; };
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
      for (int r = 0; r < n_gpus && ok; ++r) {
        vic::ViCalibrator& rc = *cals[r];
        rc.ReportCompute(report_bx, report_by);
        const std::vector<const Detection*>& dets = rank_corners[r];
        const vic::ViCalibrator::ReportViews v = rc.GetReportViews();
        for (size_t i = 0; i < v.frame.size(); ++i) {
          const long wc = (long)v.worst_corner[i];
          const long fid = frame_ids[frame_ids.size() * (size_t)r / (size_t)n_gpus + (size_t)v.frame[i]];      // (the rank's local frame -> id as in the input)
          views.push_back(ViewRow{fid, v.camera[i], v.count[i], v.removed[i], v.count[i] > 0 ? std::sqrt(v.sum_sq[i] / (2.0 * v.count[i])) : 0.0, v.max_err[i],
                                  wc >= 0 ? dets[(size_t)wc]->dot : -1});
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
          const size_t lo = frame_ids.size() * (size_t)r / (size_t)n_gpus;
          for (size_t s = 0; s < nb && fi; ++s) {
            std::fprintf(fi, "%ld,%.9f", frame_ids[lo + s], rc.GetFrame(s).time);
            for (int k = 0; k < 9; ++k) std::fprintf(fi, ",%.10g", w[9 * s + k]);
            for (int k = 0; k < 9; ++k) std::fprintf(fi, ",%.10g", u[9 * s + k]);
            std::fprintf(fi, ",%d\n", (int)fl[s]);
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
  SelectHeld select_held;
  if (!held_ids.empty()) {
    try {
      std::map<long, int> held_index;
      for (size_t i = 0; i < held_ids.size(); ++i) held_index[held_ids[i]] = (int)i;
      std::vector<int> tile_frame, tile_cam, point_id;
      std::vector<long long> tile_off(1, 0);
      std::vector<double> points, pc;
      std::vector<const Detection*> dets;
      for (size_t c = 0; c < n_cam; ++c) {
        std::map<int, std::vector<const Detection*>> per_frame;
        for (const Detection& d : channels[c].det) {
          auto it = held_index.find(d.frame);
          if (it == held_index.end() || d.dot >= grid_w * grid_h) continue;
          per_frame[it->second].push_back(&d);
        }
        for (const auto& kv : per_frame) {
          for (const Detection* d : kv.second) {
            point_id.push_back((int)dets.size());
            points.insert(points.end(), {d->X, d->Y, d->Z}); pc.insert(pc.end(), {d->u, d->v});
            dets.push_back(d);
          }
          tile_frame.push_back(kv.first); tile_cam.push_back((int)c); tile_off.push_back((long long)dets.size());
        }
      }
      // (a held-out frame nobody detected the target in still is a frame of the set)
      tile_frame.push_back((int)held_ids.size() - 1); tile_cam.push_back(0); tile_off.push_back((long long)dets.size());
      cal.HoldoutClear();
      cal.HoldoutAddTiles((int)tile_frame.size(), tile_frame.data(), tile_cam.data(), tile_off.data(), points.data(), (int)dets.size(), point_id.data(), pc.data());
      cal.HoldoutCompute(nullptr, 0);
      const vic::ViCalibrator::HoldoutFrames hf = cal.GetHoldoutFrames();
      if (select.k > 0) {
        select_held.tile_frame = tile_frame; select_held.tile_cam = tile_cam; select_held.tile_off = tile_off; select_held.point_id = point_id; select_held.points = points;
        select_held.status = hf.status;
        for (const vic::Se3& T : hf.T_wk) select_held.T_wk.insert(select_held.T_wk.end(), T.data(), T.data() + 7);
      }
      const vic::ViCalibrator::HoldoutViews hv = cal.GetHoldoutViews();
      const vic::ViCalibrator::HoldoutCameraRmse hr = cal.GetHoldoutCameraRmse();
      for (size_t c = 0; c < n_cam; ++c) {
        int k = 0;
        for (size_t i = 0; i < hv.frame.size(); ++i) k += (hv.camera[i] == (int)c && hf.status[hv.frame[i]] <= 1) ? 1 : 0;
        std::printf("Camera %zu: fitted RMSE %.6g px, held-out RMSE %.6g px over %d views, %lld corners\n", c, rmse[c], hr.rmse[c], k, hr.count[c]);
      }
      int by_status[5] = {0, 0, 0, 0, 0};
      for (int st : hf.status) if (st >= 0 && st < 5) ++by_status[st];
      std::printf("held-out frames: %zu (every %d.)", held_ids.size(), holdout_every);
      for (int st = 0; st < 5; ++st) if (by_status[st] || st == 0) std::printf("%s %d %s", st ? "," : ":", by_status[st], HoldoutStatusName(st));
      std::printf("\n");
      const std::string dir = FlagString("report_dir");
      if (!dir.empty()) {
        (void)mkdir(dir.c_str(), 0777);
        if (FILE* f = std::fopen((dir + "/holdout_views.csv").c_str(), "w")) {
          std::fprintf(f, "frame,camera,corners,rmse_px,max_px,status,iterations\n");
          for (size_t i = 0; i < hv.frame.size(); ++i)
            std::fprintf(f, "%ld,%d,%d,%.10g,%.10g,%s,%d\n", held_ids[(size_t)hv.frame[i]], hv.camera[i], hv.count[i],
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
      }
    } catch (const std::exception& e) { std::fprintf(stderr, "E held-out scoring failed: %s\n", e.what()); }
  }

  // ---- WriteCalibration (vicalib-engine.cc:353-372) + poses.csv (:407-421) ----------------------------------------------
  cal.WriteCameraModels(FlagString("output"));
  bool undistort_failed = false;
  if (!FlagString("undistort_dir").empty()) {
    if (!from_images) std::fprintf(stderr, "W -undistort_dir needs image input (-cam file://...): nothing to undistort\n");
    else {
      try {
        if (!UndistortInputs(cal, cam_files, input_cameras, calibrate_imu, (int)FlagInt("device"), FlagString("undistort_dir"), FlagDouble("undistort_alpha"), &err))
          { std::fprintf(stderr, "E undistortion failed: %s\n", err.c_str()); undistort_failed = true; }
      } catch (const std::exception& e) { std::fprintf(stderr, "E undistortion failed: %s\n", e.what()); undistort_failed = true; }
    }
  }
  bool rectify_failed = false;
  if (!FlagString("rectify_dir").empty()) {
    try {
      if (!RectifyOutputs(cal, channels, frame_ids, grid_w * grid_h, cam_files, from_images, input_cameras, calibrate_imu, (int)FlagInt("device"), FlagString("rectify_dir"),
                          rectify_a, rectify_b, FlagDouble("rectify_alpha"), &err))
        { std::fprintf(stderr, "E rectification failed: %s\n", err.c_str()); rectify_failed = true; }
    } catch (const std::exception& e) { std::fprintf(stderr, "E rectification failed: %s\n", e.what()); rectify_failed = true; }
  }
  bool compare_failed = false;
  if (!compare_b.empty()) {                              // -compare_to: the result (A) against the file (B)
    std::vector<vic::CameraAndPose> a;
    for (size_t c = 0; c < n_cam; ++c) {
      vic::CameraAndPose now = cal.GetCamera(c);
      now.model = input_cameras[c].model; now.width = input_cameras[c].width; now.height = input_cameras[c].height;
      a.push_back(now);
    }
    if (CompareRigs(a, compare_b, compare, (int)FlagInt("device"), &err) != 0) { std::fprintf(stderr, "E comparison failed: %s\n", err.c_str()); compare_failed = true; }
  }
  bool uncertainty_failed = false;
  if (!uncertainty.dir.empty()) {                        // -uncertainty_dir: the covariance at the result (collective when the frames are sharded), mapped per camera
    std::vector<std::vector<double>> covs((size_t)n_gpus);
    std::vector<int> dims((size_t)n_gpus, 0);
    std::vector<std::thread> th;
    for (int r = 0; r < n_gpus; ++r) th.emplace_back([&, r] { covs[r] = cals[r]->GetSolutionCovariance(&dims[r]); });
    for (auto& t : th) t.join();
    std::vector<vic::CameraAndPose> a;
    for (size_t c = 0; c < n_cam; ++c) {
      vic::CameraAndPose now = cal.GetCamera(c);
      now.model = input_cameras[c].model; now.width = input_cameras[c].width; now.height = input_cameras[c].height;
      a.push_back(now);
    }
    if (covs[0].empty()) { std::fprintf(stderr, "E uncertainty map failed: the solution covariance cannot be computed\n"); uncertainty_failed = true; }
    else if (!UncertaintyOutputs(a, covs[0], dims[0], rmse, uncertainty, (int)FlagInt("device"), &err)) { std::fprintf(stderr, "E uncertainty map failed: %s\n", err.c_str()); uncertainty_failed = true; }
  }
  bool stereo_uncertainty_failed = false;
  if (!stereo_uncertainty.dir.empty()) {                 // -stereo_uncertainty_dir: the covariance at the result (collective when the frames are sharded), mapped for the pair
    std::vector<std::vector<double>> covs((size_t)n_gpus);
    std::vector<int> dims((size_t)n_gpus, 0);
    std::vector<std::thread> th;
    for (int r = 0; r < n_gpus; ++r) th.emplace_back([&, r] { covs[r] = cals[r]->GetSolutionCovariance(&dims[r]); });
    for (auto& t : th) t.join();
    std::vector<vic::CameraAndPose> a;
    for (size_t c = 0; c < n_cam; ++c) {
      vic::CameraAndPose now = cal.GetCamera(c);
      now.model = input_cameras[c].model; now.width = input_cameras[c].width; now.height = input_cameras[c].height;
      a.push_back(now);
    }
    if (covs[0].empty()) { std::fprintf(stderr, "E stereo uncertainty map failed: the solution covariance cannot be computed\n"); stereo_uncertainty_failed = true; }
    else if (!StereoUncertaintyOutputs(a, covs[0], dims[0], rmse, stereo_uncertainty, (int)FlagInt("device"), &err)) { std::fprintf(stderr, "E stereo uncertainty map failed: %s\n", err.c_str()); stereo_uncertainty_failed = true; }
  }
  bool select_failed = false;
  if (select.k > 0) {                                  // -select_views: the most informative of the calibrated frames, at the result
    try {
      if (!SelectOutputs(cal, frame_ids, held_ids, select_held, select, &err)) { std::fprintf(stderr, "E view selection failed: %s\n", err.c_str()); select_failed = true; }
    } catch (const std::exception& e) { std::fprintf(stderr, "E view selection failed: %s\n", e.what()); select_failed = true; }
  }
  bool convert_failed = false;
  if (converting) {                                      // -convert_to: the cameras just written, converted
    std::vector<vic::CameraAndPose> a;
    if (!ReadRigFile(FlagString("output"), &a, &err) || ConvertRig(FlagString("output"), a, convert, compare.identity ? &compare : nullptr, (int)FlagInt("device"), &err) != 0) {
      std::fprintf(stderr, "E conversion failed: %s\n", err.c_str()); convert_failed = true;
    }
  }
  bool register_failed = false;
  if (reg.on) {                                          // -register_depth: with the cameras just written
    std::vector<vic::CameraAndPose> a;
    if (!ReadRigFile(FlagString("output"), &a, &err) || RegisterRig(a, reg, (int)FlagInt("device"), &err) != 0) {
      std::fprintf(stderr, "E registration failed: %s\n", err.c_str()); register_failed = true;
    }
  }
  bool depthcal_failed = false;
  if (depthcal.on) {                                     // -depthcal_depth: with the cameras just written and the poses of the calibration's frames, in their order
    std::vector<vic::CameraAndPose> a;
    std::vector<std::array<double, 7>> poses;
    for (size_t i = 0; i < all_frames.size(); ++i) { std::array<double, 7> T; for (int k = 0; k < 7; ++k) T[k] = all_frames[i].t_wp_.v[k]; poses.push_back(T); }
    if (!ReadRigFile(FlagString("output"), &a, &err) || DepthCalFit(a, poses, "the calibration", depthcal, (int)FlagInt("device"), &err) != 0) {
      std::fprintf(stderr, "E depth calibration failed: %s\n", err.c_str()); depthcal_failed = true;
    }
  }
  if (FlagBool("print_poses")) {
    if (FILE* f = std::fopen("poses.txt", "w")) {
      for (size_t i = 0; i < all_frames.size(); ++i) { double c[6]; T2Cart(all_frames[i].t_wp_.data(), c); std::fprintf(f, "%f\t%f\t%f\t%f\t%f\t%f\n", c[0], c[1], c[2], c[3], c[4], c[5]); }
      std::fclose(f);
    }
  }
  if (FlagBool("save_poses")) {
    if (FILE* f = std::fopen("poses.csv", "w")) {
      std::fprintf(f, "%% Pose file generated with vicalib.\n%% Each line is the 12 elements from the top 3 rows of a 4x4transformation matrix, printed row major.\n");
      for (size_t i = 0; i < all_frames.size(); ++i) {
        const vic::VicalibFrame& fr = all_frames[i];
        double R[9]; RotationMatrix(fr.t_wp_.data(), R);
        std::fprintf(f, "%.10g %.10g %.10g %.10g     %.10g %.10g %.10g %.10g     %.10g %.10g %.10g %.10g\n", R[0], R[1], R[2], fr.t_wp_.v[4], R[3], R[4], R[5], fr.t_wp_.v[5], R[6], R[7], R[8], fr.t_wp_.v[6]);
      }
      std::fclose(f);
    }
  }
  // ---- IsSuccessful (vicalib-task.cc:831-856) ------------------------------------------------------------------------------
  bool success = true;
  for (size_t c = 0; c < n_cam; ++c)
    if (!(rmse[c] <= FlagDouble("max_reprojection_error"))) {
      std::fprintf(stderr, "W Reprojection error of %g was greater than maximum of %g for camera %zu\n", rmse[c], FlagDouble("max_reprojection_error"), c);
      success = false;
    }
  if (success && guess) for (size_t c = 0; c < n_cam; ++c) {
    vic::CameraAndPose now = cal.GetCamera(c); now.model = input_cameras[c].model;
    if (CameraCalibrationsDiffer(input_cameras[c], now)) { success = false; break; }
  }
  if (success && guess) {                        // vicalib-task.cc:852-853 (input_imu_biases_: the calibrator's biases at construction, :129)
    const double input_imu_biases[6] = {0, 0, 0, 0, 0, 0};
    const auto bias_now = cal.GetBiases();
    if (IMUCalibrationDiffer(input_imu_biases, bias_now.data(), FlagString("imu_diff_sense") != "corrected")) success = false;
  }
  std::printf("calibration %s -> %s\n", success ? "succeeded" : "FAILED", FlagString("output").c_str());
  if (undistort_failed) std::fprintf(stderr, "E -undistort_dir: the undistorted images are incomplete (exit status %d)\n", success ? 1 : 2);
  if (rectify_failed) std::fprintf(stderr, "E -rectify_dir: the rectification's files are incomplete (exit status %d)\n", success ? 1 : 2);
  if (compare_failed) std::fprintf(stderr, "E -compare_to: the comparison's files are incomplete (exit status %d)\n", success ? 1 : 2);
  if (convert_failed) std::fprintf(stderr, "E -convert_to: the converted rig is incomplete (exit status %d)\n", success ? 1 : 2);
  if (uncertainty_failed) std::fprintf(stderr, "E -uncertainty_dir: the uncertainty map's files are incomplete (exit status %d)\n", success ? 1 : 2);
  if (stereo_uncertainty_failed) std::fprintf(stderr, "E -stereo_uncertainty_dir: the stereo uncertainty map's files are incomplete (exit status %d)\n", success ? 1 : 2);
  if (select_failed) std::fprintf(stderr, "E -select_views: the selection's files are incomplete (exit status %d)\n", success ? 1 : 2);
  if (register_failed) std::fprintf(stderr, "E -register_depth: the registered images are incomplete (exit status %d)\n", success ? 1 : 2);
  if (depthcal_failed) std::fprintf(stderr, "E -depthcal_depth: the depth correction is incomplete (exit status %d)\n", success ? 1 : 2);
  return success ? ((undistort_failed || rectify_failed || compare_failed || convert_failed || uncertainty_failed || stereo_uncertainty_failed || select_failed || register_failed || depthcal_failed) ? 1 : 0) : 2;
}
