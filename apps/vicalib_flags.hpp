// The command-line tool's flags: definitions (names, defaults and help strings of the reference tool, plus this tool's own) and the gflags-style
// parser.  A piece of vicalib.cpp's translation unit: that file includes it behind the system headers, nothing else does.
#pragma once
// ------------------------------------------------------------------------------------------- flags
struct Flag { std::string type, value, help; };
static std::map<std::string, Flag> g_flags;
static void Define(const char* name, const char* type, const char* def, const char* help) { g_flags[name] = Flag{type, def, help}; }
static bool FlagBool(const char* n) { const std::string& v = g_flags.at(n).value; return v == "true" || v == "1" || v == "yes"; }
static double FlagDouble(const char* n) { return std::atof(g_flags.at(n).value.c_str()); }
static long FlagInt(const char* n) { return std::atol(g_flags.at(n).value.c_str()); }
static const std::string& FlagString(const char* n) { return g_flags.at(n).value; }
static int Device() { return (int)FlagInt("device"); }

static void DefineEngineFlags() {      // vicalib-engine.cc:30-104
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
  Define("seed_rig", "string", "off", "off | pnp | mono.  Start the pose of every camera but the first from the views it shares with the others (a vote among the per-frame relative poses, on the GPU) instead of -model_files' pose or identity.  pnp: the poses of one PnP batch at the start intrinsics; for -model_files with good intrinsics and no poses -- at the default start intrinsics (f = 300, no distortion) this mode is biased by tens of degrees on distorted lenses.  mono: every camera is calibrated alone first, its result gives its start intrinsics and its views.");
  Define("seed_rig_tol_deg", "double", "3", "Two per-frame relative poses agree for -seed_rig within this angle, and within this angle times the distance to the target (more than 0, less than 90).");
  Define("seed_rig_min_support", "int32", "3", "-seed_rig wants at least this many agreeing frames for a pair of cameras.");
  Define("seed_rig_max_rmse", "double", "1.0", "-seed_rig mono leaves out a camera whose calibration alone ends above this many pixels of reprojection RMSE.");
  Define("seed_imu", "bool", "false", "With -imu: start the camera-IMU rotation of camera 0, the time offset, the gyro bias and gravity from the data (camera rates against gyro rates, on the GPU) instead of identity, the streams' first stamps, zero and one accelerometer sample.");
  Define("seed_imu_range", "double", "0.5", "Time offsets searched by -seed_imu: -range ... +range seconds around the start value.");
  Define("seed_imu_step", "double", "0", "Step of that search in seconds (0: the median IMU sample interval).");
  Define("seed_imu_max_gap", "double", "0.5", "Consecutive frames further apart than this many seconds give -seed_imu no rate.");
  Define("seed_imu_min_intervals", "int32", "10", "-seed_imu wants at least this many frame intervals with a rate (at least 3).");
  Define("dot_bias_rounds", "int32", "0", "After the solve, this many times: predict the bias of every dot's measured centre (the centre of a circle's image is not the image of "
         "its centre) at the result on the GPU, subtract it from the original detections and solve again from the result (0: off; needs -gpus 1, no -holdout_every).  "
         "The radii are -grid_large_rad / -grid_small_rad by the target's pattern (-grid_pattern_file, or generated from -grid_height / -grid_width / -grid_seed), or -dot_radius.");
  Define("dot_radius", "double", "0", "With -dot_bias_rounds: the radius of every dot (m), instead of the large / small pattern (0: use the pattern).");
  Define("refine_target_rounds", "int32", "0", "After the solve, this many times: refine the 3-D positions of the target's dots at the result on the GPU (one Gauss-Newton step, "
         "frame poses and shared camera parameters marginalised, position / orientation / size of the target held at the nominal one), rebuild the calibrator from the result "
         "with the refined target and solve again (0: off; needs -gpus 1, no -holdout_every, no -dot_bias_rounds, no calibrated IMU).");
  Define("refine_target_sigma", "double", "0.01", "With -refine_target_rounds: how far a dot may be expected from its nominal position (m); the prior's weight is 1 / sigma^2.");
  Define("refine_target_output", "string", "target_refined.csv", "With -refine_target_rounds: the refined target, dot,x,y,z,nx,ny,nz,corners,status per dot.");
  Define("target_points", "string", "", "A file written by -refine_target_output: the calibration starts from that measured target instead of the grid (the nominal target stays the grid).");
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
  Define("grid_large_rad", "double", "0.00423", "(pattern front-end) radius of large dots (m); read only by -dot_bias_rounds, ignored otherwise.");
  Define("grid_small_rad", "double", "0.00283", "(pattern front-end) radius of small dots (m); read only by -dot_bias_rounds, ignored otherwise.");
  Define("clip_good", "bool", "false", "(sensor front-end) ignored: output proto file of only good tracked images.");
}
static void DefineTaskFlags() {      // vicalib-task.cc:19-51, and what only this tool has up to held-out scoring
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
}
static void DefineToolFlags() {      // the outputs behind a calibration and the file-to-file tools
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
static void DefineFlags() { DefineEngineFlags(); DefineTaskFlags(); DefineToolFlags(); }

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
