/* vicalib_amd.h -- C ABI of the MI355X-native calibration solver.
 *
 * Drop-in boundary for the optimisation core of arpg/vicalib: every entry point replaces one
 * public member of visual_inertial_calibration::ViCalibrator (include/vicalib/vicalibrator.h:119-544),
 * the header-only class that VicalibTask owns by value (vicalib-task.h:120) and drives from
 * vicalib-task.cc / vicalib-engine.cc.  Plain pointers and sizes only; the library copies in and
 * copies out, the handle is opaque, and nothing aborts: every call returns a status
 * (the reference CHECK()s / LOG(FATAL)s instead, vicalibrator.h:254, :377, :396, :456).
 *
 * Conventions (same as the reference's parameter blocks):
 *   SE3  = 7 doubles [qx qy qz qw tx ty tz]   (Sophus::SE3d::data(), vicalibrator.h:460, :604)
 *   T_wk = pose of the rig ("k") in the world; T_ck maps rig coordinates into camera c
 *   intrinsics = [fu fv u0 v0 distortion...]  (calibu parameter order, vicalib-engine.cc:207-257)
 *
 * The solver needs a HIP device (gfx950).  vc_create() fails with VC_ERR_NO_DEVICE on a machine
 * without one; there is no CPU fallback.
 */
#ifndef VICALIB_AMD_H_
#define VICALIB_AMD_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vc_calibrator vc_calibrator;

enum {
  VC_OK = 0,
  VC_ERR_NO_DEVICE = -1,      /* no HIP device / HIP runtime error */
  VC_ERR_BAD_ARG = -2,        /* index out of range, null pointer, unsupported model */
  VC_ERR_RUNNING = -3,        /* setter called while the solver runs (reference: CHECK(!is_running_)) */
  VC_ERR_TIME_ORDER = -4,     /* IMU timestamps not strictly increasing (vicalibrator.h:373-378) */
  VC_ERR_TOO_MANY_POINTS = -5,/* more than 32768 distinct target points */
  VC_ERR_NUMERIC = -6,        /* factorisation failed repeatedly */
  VC_ERR_UNSUPPORTED = -7,    /* feature of the reference not available in this build */
  VC_ERR_NO_CONVERGENCE = -8  /* one stage's problem ended NO_CONVERGENCE 64 times in a row (the reference would keep
                                 cranking, vicalibrator.h:952); state and multiplicities are left as they were */
};

/* -models strings of vicalib-engine.cc:203-253, in this order */
enum { VC_MODEL_FOV = 0, VC_MODEL_POLY2 = 1, VC_MODEL_POLY3 = 2, VC_MODEL_KB4 = 3, VC_MODEL_LINEAR = 4, VC_MODEL_RATIONAL6 = 5 };

/* ViCalibrator() vicalibrator.h:124-155 + Clear() :232-249.  device = HIP ordinal. */
int vc_create(vc_calibrator** out, int device);
void vc_destroy(vc_calibrator* h);
int vc_clear(vc_calibrator* h);                                   /* Clear() :232 */

/* AddCamera(cam, T_ck) :332-342 -> camera id (>= 0) or error */
int vc_add_camera(vc_calibrator* h, int model, const double* params, int nparams, int width, int height,
                  const double T_ck[7]);
int vc_fix_camera_intrinsics(vc_calibrator* h, int should_fix);   /* FixCameraIntrinsics :346 */
/* AddFrame(T_wk, time) :355-367 -> frame id */
int vc_add_frame(vc_calibrator* h, const double T_wk[7], double time);
/* GetFrame(id)->t_wp_ = ... (vicalib-task.cc:347-348) */
int vc_set_frame_pose(vc_calibrator* h, int frame, const double T_wk[7]);
/* Pose initialisation of the frames from their detections: replaces calibu::PosePnPRansac + the pose write at
   vicalib-task.cc:335-348 (T_wk = T_cw^-1 * T_ck, camera 0 if it tracked the grid, otherwise the last camera that
   did).  Deterministic planar homography + LM refinement on the current intrinsics; host code, runs once. */
int vc_init_frame_poses_pnp(vc_calibrator* h, int* n_initialised);
/* The same for one view, no handle: T_cw of a camera of `model`/`params` seeing n >= 4 corners of the planar grid. */
int vc_pnp_planar(int model, const double* params, int nparams, int n, const double* p_w /* n x 3 */,
                  const double* p_c /* n x 2 */, double T_cw[7], double* rms_px);
/* The robust branch of PosePnPRansac (robust_3pt_its > 0; the reference passes 0, 0 at vicalib-task.cc:323-325, which is
   vc_pnp_planar): `iterations` minimal 4-corner samples, consensus at tol_px pixels of reprojection error on the full camera
   model, refit on the consensus set.  inlier (n flags) and n_inliers are optional.  vc_set_pnp_ransac makes
   vc_init_frame_poses_pnp use it (iterations = 0 restores the reference's call). */
int vc_pnp_planar_ransac(int model, const double* params, int nparams, int n, const double* p_w, const double* p_c,
                         int iterations, double tol_px, double T_cw[7], double* rms_px, int* n_inliers, char* inlier);
int vc_set_pnp_ransac(vc_calibrator* h, int iterations, double tol_px);
/* Poses of many views of the planar target at once, on the device.  View v owns corners view_off[v] .. view_off[v+1]-1.
   One wavefront per view runs what vc_pnp_planar_ransac runs (iterations = 0 or a view of fewer than 5 corners: vc_pnp_planar).
   status[v]: 0 ok, 1 fewer than 4 corners, 2 not planar, 3 no pose (DLT / rotation / refinement failed), 4 no consensus (< 4 inliers).
   T_cw, rms, n_inliers of a view with status != 0 are left untouched; inlier (may be NULL) gets 0 there.
   VC_ERR_BAD_ARG before any device call (a null pointer, n_views < 0, offsets that decrease, an unknown model, iterations < 0,
   a tol_px that is not >= 0); VC_ERR_NO_DEVICE without that device.  Two runs, and a view alone or among others, give the same bits. */
int vc_pnp_planar_batch(int device, int n_views, const int* view_model, const double* view_K /* n_views x 10 */,
                        const int* view_off /* n_views + 1 */, const double* p_w /* total x 3 */, const double* p_c /* total x 2 */,
                        int iterations, double tol_px, double* T_cw /* n_views x 7 */, double* rms, int* n_inliers,
                        char* inlier /* total, or NULL */, int* status);
/* Mean time in ms of the batch's kernel alone on that input: `reps` launches back to back between two events, after one run that warms up. */
int vc_time_pnp_planar_batch(int device, int n_views, const int* view_model, const double* view_K, const int* view_off, const double* p_w,
                             const double* p_c, int iterations, double tol_px, int reps, double* kernel_ms);
/* on: vc_init_frame_poses_pnp and the seeds of vc_holdout_compute(h, NULL, ...) come from one vc_pnp_planar_batch over every view of
   >= 4 corners on the calibrator's device; the rule that picks a frame's camera stays on the host.  Default 0: the host routine. */
int vc_set_pnp_device(vc_calibrator* h, int on);
/* The focal length of every camera from its views of the planar target, on the device, before anything is solved: a start value for
   fx = fy where no model file gives one.  View v belongs to camera view_cam[v] and owns corners view_off[v] .. view_off[v+1]-1.
   A corner is used when both coordinates are finite and it lies within cam_radius pixels of the camera's assumed principal point
   cam_pp (radius <= 0: every finite corner).  Per view: H, the DLT homography from target (X, Y) to pixel - principal point, scaled
   to h1x^2 + h1y^2 + h2x^2 + h2y^2 = 2 (h1, h2: its first two columns); view_rows = c1 d1 c2 d2 with c1 = h1x h2x + h1y h2y,
   d1 = -h1z h2z, c2 = (h1x^2 + h1y^2) - (h2x^2 + h2y^2), d2 = h2z^2 - h1z^2, so that c1 / f^2 = d1 and c2 / f^2 = d2;
   view_f = the focal length of that view alone (NaN when the view is tilted by less than min_tilt_deg or gives none; diagnosis only);
   view_fit_px = the rms transfer error of H over the used corners.
   view_status: 0 ok, 1 fewer than max(min_corners, 4) used corners, 2 used target points not on one plane z, 3 no homography,
   4 view_fit_px above max_fit_px (max_fit_px = 0: not tested).  The outputs of a view with status != 0 are left untouched.
   Per camera, over its status-0 views in view order: Scc = sum(c1^2 + c2^2), Scd = sum(c1 d1 + c2 d2), cam_f = sqrt(Scc / Scd);
   cam_views = the number of those views.  cam_status: 0 ok, 1 no usable view, 2 Scc < sin^4(min_tilt_deg) (the target was never
   tilted), 3 Scd / Scc not positive or not finite.  cam_f of a camera with status != 0 is left untouched.
   VC_ERR_BAD_ARG before any device call (a null pointer other than view_H, n_views < 0, n_cams < 1, a view_cam outside
   0 .. n_cams-1, offsets that decrease, a principal point that is not finite, max_fit_px < 0, min_tilt_deg outside (0, 90));
   VC_ERR_NO_DEVICE without that device: there is no host fallback.  Two runs give the same bits, a view gives the same bits alone
   or among others, and a camera's result does not depend on the views of other cameras in the batch. */
int vc_seed_focal_batch(int device, int n_views, const int* view_cam, int n_cams,
                        const double* cam_pp /* n_cams x 2 */, const double* cam_radius /* n_cams */,
                        const int* view_off /* n_views + 1 */, const double* p_w /* total x 3 */,
                        const double* p_c /* total x 2 */, int min_corners, double max_fit_px, double min_tilt_deg,
                        double* view_H /* n_views x 9, may be NULL */,
                        double* view_rows /* n_views x 4: c1 d1 c2 d2 */,
                        double* view_f, double* view_fit_px, int* view_used, int* view_status,
                        double* cam_f, int* cam_views, int* cam_status);
/* Mean time in ms of the batch's two kernels alone on that input: `reps` runs back to back between two events, after one that warms up. */
int vc_time_seed_focal_batch(int device, int n_views, const int* view_cam, int n_cams, const double* cam_pp, const double* cam_radius,
                             const int* view_off, const double* p_w, const double* p_c, int min_corners, double max_fit_px,
                             double min_tilt_deg, int reps, double* kernel_ms);
/* The predicted bias of a dot's measured centre, on the device.  A measurement is the centre of the dot's image ellipse as the detector's
   dual-conic fit returns it; the solve holds it against the projection of the circle's centre, and under perspective and distortion the two
   differ.  View v has the camera (view_model, view_K) and the pose view_T_cw (target into camera, [qx qy qz qw tx ty tz]) and owns
   observations view_off[v] .. view_off[v+1]-1.  An observation is a dot centre p_w on the target and its radius in metres; the circle lies
   in the plane through the centre parallel to the target's x-y plane.  bias = what the detector's estimator (unit weights, 64 samples of
   the rim, no noise, no blur) returns minus project(centre), in pixels: subtract it from a measurement.  radius_px = the dot's radius in
   pixels to first order.  status: 0 ok, 1 the centre does not project (behind the camera, not finite), 2 a rim sample does not project or
   its edge direction is zero or not finite, 3 the 5 x 5 system is singular or the bias is not finite, 4 |bias| > radius_px (the estimate
   left the dot: the view is too oblique to trust).  The outputs of an observation with status != 0 are left untouched.  radius = 0: bias
   exactly (0, 0), radius_px 0, status 0 (where the centre projects).
   VC_ERR_BAD_ARG before any device call (a null pointer, n_views < 0, offsets that decrease or start below 0, an unknown model, a radius
   that is negative or not finite); VC_ERR_NO_DEVICE without that device: there is no host fallback.  Two runs give the same bits, and an
   observation gives the same bits alone or among others. */
int vc_dot_bias_batch(int device, int n_views, const int* view_model, const double* view_K /* n_views x 10 */,
                      const double* view_T_cw /* n_views x 7 */, const int* view_off /* n_views + 1 */,
                      const double* p_w /* total x 3 */, const double* radius /* total */,
                      double* bias /* total x 2 */, double* radius_px /* total */, int* status /* total */);
/* Mean time in ms of the batch's kernel alone on that input: `reps` launches back to back between two events, after one that warms up. */
int vc_time_dot_bias_batch(int device, int n_views, const int* view_model, const double* view_K, const double* view_T_cw, const int* view_off,
                           const double* p_w, const double* radius, int reps, double* kernel_ms);
/* One Gauss-Newton step on the calibration target's points with the frame poses AND the shared camera columns marginalised, on the device
   (vicalib_amd/csrc/vc_target_refine.hpp has the definition).  The rig is that of vc_selector_create: n_cameras <= 8 cameras
   (model, params x 10, T_ck x 7, cam_flags = kCamRotFree 1 | kCamTransFree 2 | kCamKFree 4, the shared columns D = sum of the cameras' free
   columns <= 64, D = 0 allowed); n_frames poses T_wk (x 7); tile t holds corners tile_off[t] .. tile_off[t+1]-1 of point_id / p_c (measured
   pixels, x 2) of (tile_frame[t], tile_cam[t]); points is the current target and nominal the printed one (n_points x 3 each,
   4 <= n_points <= 1024); lambda > 0 is the prior's weight in px^2 / m^2 on the offset from nominal.  Corner rows are at unit weight, without
   robust loss; a corner at camera depth <= 0 (any model but kb4) enters nothing and is counted behind.  frame_status: n_frames x
   [status, corners, behind], status 0 usable, 1 underdetermined (fewer than 4 corners or a pivot of J_f^T J_f at or below 1e-12 x its largest
   diagonal entry: the frame adds nothing), 2 usable with corners behind.  point_status: 0 refined, 1 no usable corner (left out of the system
   and of the gauge; its row of refined is its row of points, bit for bit); point_corners: the usable corners of every point.  The similarity
   tangent at nominal about the observed points' centroid is projected out: Q^T (refined - nominal) = 0, gauge_rank is the number of its
   columns kept (7 unless the observed points are degenerate).  result_status: 0 ok, 1 singular (a pivot of the dense factorisation at or
   below 1e-12 x the largest diagonal entry: refined, cost and predicted_decrease are left untouched).  cost = 1/2 sum r^2 over the usable
   corners; predicted_decrease = 1/2 d . (Pi b).
   VC_ERR_BAD_ARG before any device call (a null pointer, offsets that decrease or start below 0, a frame, camera or point id out of range,
   an unknown model or flag, values that are not finite, lambda not finite and positive, n_points < 4); VC_ERR_UNSUPPORTED for D > 64,
   n_points > 1024 or n_frames > 2^20; VC_ERR_NO_DEVICE without that device or when a HIP call fails (device memory included: the dense system is
   (3 n_points)^2 doubles, 75 MB at the limit, the (frame, point) table n_frames x n_points ints): there is no host fallback.  No floating-point atomic: two runs give the same bits. */
int vc_target_refine_batch(int device, int n_cameras, const int* model, const double* params /* n_cameras x 10 */,
                           const double* T_ck /* n_cameras x 7 */, const int* cam_flags, int n_frames, const double* T_wk /* n_frames x 7 */,
                           int n_tiles, const int* tile_frame, const int* tile_cam, const long long* tile_off /* n_tiles + 1 */,
                           const int* point_id, const double* p_c /* x 2 */, const double* points /* n_points x 3 */,
                           const double* nominal /* n_points x 3 */, int n_points, double lambda, double* refined /* n_points x 3 */,
                           int* point_status, int* point_corners, int* frame_status /* n_frames x 3 */, int* gauge_rank, int* result_status,
                           double* cost, double* predicted_decrease);
/* Mean time in ms of the step's six stages alone on that input (sweep, assembly, elimination of the shared columns, gauge, factorisation,
   solve): `reps` runs of the whole step with events between the stages, after one run that warms up.  kernel_ms: 6 doubles. */
int vc_time_target_refine_batch(int device, int n_cameras, const int* model, const double* params, const double* T_ck, const int* cam_flags,
                                int n_frames, const double* T_wk, int n_tiles, const int* tile_frame, const int* tile_cam,
                                const long long* tile_off, const int* point_id, const double* p_c, const double* points, const double* nominal,
                                int n_points, double lambda, int reps, double* kernel_ms /* 6 */);
/* AddObservation(frame, cam, p_w, p_c, time) :385-468, in bulk: n corners of one (frame, camera) */
int vc_add_observations(vc_calibrator* h, int frame, int camera, int n, const double* p_w /* n x 3 */,
                        const double* p_c /* n x 2 */);
/* The same over many (frame, camera) groups in one call, target points by index: group t holds corners
 * [tile_off[t], tile_off[t+1]) of point_id / p_c; points is the caller's table of target points (n_points x 3). */
int vc_add_observation_tiles(vc_calibrator* h, int n_tiles, const int* tile_frame, const int* tile_cam,
                             const long long* tile_off /* n_tiles + 1 */, const double* points, int n_points,
                             const int* point_id, const double* p_c /* x 2 */);
/* AddImuMeasurements(gyro, accel, time) :370-380, in bulk */
int vc_add_imu(vc_calibrator* h, int n, const double* gyro /* n x 3 */, const double* accel /* n x 3 */,
               const double* time /* n */);

int vc_set_sigmas(vc_calibrator* h, double gyro_sigma, double accel_sigma);       /* SetSigmas :290 */
int vc_set_biases(vc_calibrator* h, const double biases[6]);                       /* SetBiases :301 */
int vc_set_scale_factor(vc_calibrator* h, const double scale[6]);                  /* SetScaleFactor :308 */
int vc_set_time_offset(vc_calibrator* h, double offset);                           /* SetTimeOffset :296 */
int vc_set_function_tolerance(vc_calibrator* h, double tol);                       /* SetFunctionTolerance :277 */
/* SetOptimizationFlags(bias_active, inertial_active, rotation_only, optimize_imu_time_offset) :252-260 */
int vc_set_optimization_flags(vc_calibrator* h, int bias_active, int inertial_active, int rotation_only,
                              int optimize_time_offset);
/* gflags read inside the calibrator: FLAGS_max_iters (:142), FLAGS_calibrate_imu (:214, :651, :977),
 * FLAGS_remove_outliers / FLAGS_outlier_threshold (:870, :995, :1024) */
int vc_set_max_iters(vc_calibrator* h, int max_iters);
/* ceres::Solver::Options::gradient_tolerance / parameter_tolerance, which the reference leaves at the Ceres defaults
 * (1e-10 / 1e-8, vicalibrator.h:141-151); settable here so that tests can converge a solve to rounding level */
int vc_set_tolerances(vc_calibrator* h, double gradient_tolerance, double parameter_tolerance);
int vc_set_calibrate_imu(vc_calibrator* h, int calibrate_imu);
int vc_set_remove_outliers(vc_calibrator* h, int remove_outliers, double outlier_threshold);

/* Start() :263 / IsRunning() :314 / Stop() :317; vc_solve = Start() + join (blocking SolveThread :919) */
int vc_solve(vc_calibrator* h);
int vc_start(vc_calibrator* h);
/* is_finished_ is sticky until Clear() as in the reference (:246, :922): Start()/Solve() on a finished calibrator return at
 * once.  vc_resume clears the flag (engine-level, no reference counterpart) so that the next Solve() runs SetupProblem +
 * the solve loop again from the current state (re-adding every block once more, as any pass of the outer loop does). */
int vc_resume(vc_calibrator* h);
/* Bench / test hook: Solve() runs the first n stages of the schedule (:977-1000), sets up stage n + 1 (constancy flags,
 * block multiplicities, gravity) and returns without running it; n < 0 (default) = the whole schedule.  With the state
 * left there, vc_prepare + vc_run_iterations time LM iterations of exactly that stage. */
int vc_set_stage_limit(vc_calibrator* h, int n);
int vc_is_running(vc_calibrator* h);
int vc_stop(vc_calibrator* h);

/* readers (fields of CalibrationStats, calibration-stats.h:34-42) */
int vc_num_frames(vc_calibrator* h);                                               /* NumFrames :471 */
/* IMU blocks this rank owns (0 without inertial terms): one per own frame that has a successor.  On a frame-sharded visual-inertial
 * calibrator every rank but the last also owns the block that ends in the next rank's separator, of which it keeps a ghost copy:
 * vc_num_frames - 1, plus 1 on those ranks (VC_ERR_BAD_ARG for a sharded rank of fewer than 2 frames, which the upload refuses).
 * vc_get_imu_blocks and vc_get_imu_weights write the blocks of the last upload, never more than this count. */
int vc_num_imu_blocks(vc_calibrator* h);
int vc_num_cameras(vc_calibrator* h);                                              /* NumCameras :484 */
int vc_get_camera(vc_calibrator* h, int camera, double* params, int* nparams, double T_ck[7]);   /* GetCamera :492 */
int vc_get_frame(vc_calibrator* h, int frame, double T_wk[7], double v_w[3], double* time);      /* GetFrame :477 */
int vc_get_biases(vc_calibrator* h, double biases[6]);                             /* GetBiases :286 */
int vc_get_scale_factor(vc_calibrator* h, double scale[6]);                        /* GetScaleFactor :306 */
int vc_get_gravity(vc_calibrator* h, double g_dir[2]);                             /* imu_.g_ :1020 */
double vc_time_offset(vc_calibrator* h);                                           /* time_offset :474 */
double vc_mean_squared_error(vc_calibrator* h);                                    /* MeanSquaredError :506 */
int vc_get_camera_proj_rmse(vc_calibrator* h, double* rmse /* n_cameras */);       /* GetCameraProjRMSE :160 */
unsigned vc_get_num_iterations(vc_calibrator* h);                                  /* GetNumIterations :283 */
/* imu_buffer() :487: the stored measurements in time order (any pointer may be NULL); returns the number copied */
int vc_num_imu_measurements(vc_calibrator* h);
int vc_get_imu_measurements(vc_calibrator* h, double* gyro, double* accel, double* time, int max_n);
/* GetIntegrationPoses(id) :508-533: the poses the IMU integration passes through between frame id and id + 1 -- the start pose,
 * then one per measurement of the range; rows of 11 doubles [q(4) t(3) v_w(3) time].  Returns the count (0 unless the inertial
 * terms are fully active, :510), which may exceed max_poses. */
int vc_get_integration_poses(vc_calibrator* h, int id, double* poses, int max_poses);
/* PrintResults() :536-544 into buf: per camera its parameters and T_ck as a 4 x 4 matrix; returns the length of the text.
 * len = 0 (buf may be NULL): only the length is returned -- the text needs a buffer of that + 1 bytes; a buffer too small is VC_ERR_BAD_ARG */
int vc_print_results(vc_calibrator* h, char* buf, int len);
/* WriteCameraModels(filename) :208-229 (calibu rig XML) */
int vc_write_camera_models(vc_calibrator* h, const char* filename);

/* GetSolutionCovariance(problem) :802-857 (compiled in the reference only with COMPUTE_VICALIB_COVARIANCE, :1004-1013):
 * covariance of the blocks of covariance_params_ (:561, :567, :594) at the current state -- per camera q_ck (4, lifted
 * through the SO3 local parameterisation), p_ck (3) and, unless the intrinsics are fixed, the model parameters; frames
 * and IMU states marginalised; constant blocks are zero.  n x n row-major, n = vc_solution_covariance_dim().
 * The names string is the reference's column header ("c[0].q_ck:(4) c[0].p_ck:(3) c[0].params:(5) ..."). */
int vc_solution_covariance_dim(vc_calibrator* h);
int vc_get_solution_covariance(vc_calibrator* h, double* cov, int max_n, int* n);
int vc_get_solution_covariance_names(vc_calibrator* h, char* buf, int len);

/* ---- engine-level entry points (no counterpart in the reference: it has no GPU, no sharding) ---- */
/* State the reference keeps inside the class with no setter (imu_.g_, VicalibFrame::v_w_): start values for tests and for a
 * caller that resumes from a stored calibration.  vc_set_gravity also marks gravity as initialised (:927-949 is skipped). */
int vc_set_gravity(vc_calibrator* h, const double g_dir[2]);
int vc_set_frame_velocities(vc_calibrator* h, const double* v_w /* n x 3 */, int n);
/* Per-iteration record of the trust-region loop = the columns of the reference's log line (:698-707).
 * rows of 10 doubles: iteration, cost, cost_change, gradient_max_norm, gradient_norm, step_norm,
 * relative_decrease, trust_region_radius, accepted, stage */
int vc_trace_len(vc_calibrator* h);
int vc_get_trace(vc_calibrator* h, double* rows, int max_rows);
/* Frame sharding across processes (one process per GPU): this handle holds frames
 * [first_global_frame, first_global_frame + n_local) of a problem that world_size ranks solve together.
 * allreduce_sum / allreduce_max are called on every LM iteration with a DEVICE pointer and must return
 * only when the reduction is complete on the calibrator's stream (see vc_get_stream). */
typedef int (*vc_allreduce_fn)(void* ctx, double* device_buf, int count, int op /*0 sum, 1 max*/);
int vc_set_shard(vc_calibrator* h, int rank, int world_size, vc_allreduce_fn fn, void* ctx);
void* vc_get_stream(vc_calibrator* h);    /* hipStream_t */
/* The same sharding with the library's own RCCL communicator (librccl bound at run time): the per-iteration all-reduces
 * are enqueued directly on the calibrator's stream, no callback.  Rank 0 creates the id (ncclGetUniqueId, 128 bytes),
 * the host distributes it by whatever means it has, every rank calls vc_set_shard_rccl (collective: ncclCommInitRank). */
int vc_rccl_unique_id(void* out128);
int vc_set_shard_rccl(vc_calibrator* h, int rank, int world_size, const void* unique_id128);
/* One RCCL communicator for several calibrators of a process (a launcher that solves more than once: one ncclCommInitRank and
 * one ncclCommDestroy per process instead of one pair per calibrator).  vc_shard_comm_create is collective like
 * vc_set_shard_rccl; vc_set_shard_comm lends the communicator to a calibrator on the same device (rank / world size are the
 * communicator's); the caller destroys it after the calibrators that used it. */
typedef struct vc_shard_comm vc_shard_comm;
int vc_shard_comm_create(int device, int rank, int world_size, const void* unique_id128, vc_shard_comm** out);
int vc_set_shard_comm(vc_calibrator* h, vc_shard_comm* comm);
void vc_shard_comm_destroy(vc_shard_comm* comm);
long long vc_allreduce_calls(vc_calibrator* h);    /* all-reduces issued through the library's own communicator */
/* The sharding a calibrator runs with: rank / world_size as set by vc_set_shard*, and -- for the library's own communicator -- what
 * RCCL itself reports (ncclCommCount, ncclCommUserRank; -1: no RCCL communicator attached): a launcher can check that RCCL saw the
 * ranks it was started with.  Any of the pointers may be NULL.  (The reference is single-process: vicalibrator.h:263-274.) */
int vc_shard_info(vc_calibrator* h, int* rank, int* world_size, int* rccl_ranks, int* rccl_rank);
/* Which forms of the visual-inertial pass the uploaded problem runs (after vc_prepare / a solve; a parity hook: the tests assert that the
 * kernels they mean to check are the ones that ran): out6 = { chain assembly folded into the bottom level (k_chain_l0), back-substitution as
 * one launch (k_chain_back_path), Gram sums in the top level's launch, top-level frames as a partial record of their own, the reduced
 * solve's tail in the back-substitution's launch, the shared parameters' blocks formed ahead of the reduced solve }. */
int vc_pass_paths(vc_calibrator* h, int* out6);
/* Which levels of the chain elimination the uploaded problem eliminates by odd-even reduction inside a workgroup (same standing as
 * vc_pass_paths): *n_levels = levels below the top one, oe_levels[l] (l < cap; the caller provides cap ints) = 1 where level l does,
 * *oe_top likewise for the top level. */
int vc_chain_order(vc_calibrator* h, int* n_levels, int* oe_levels, int cap, int* oe_top);
/* Text behind the last failing status of vc_set_shard_rccl on this thread (which library call failed, RCCL's error string and
 * last-error text): what a launcher prints before it falls back to another transport.  Empty if nothing failed. */
const char* vc_last_error(void);
/* Upload the problem and linearise once at the current state (stage flags as set): fills the device
 * normal equations.  Used by the parity tests and the benchmark. */
int vc_prepare(vc_calibrator* h);
/* Copies of device results after vc_prepare / vc_linearize (any pointer may be NULL):
 *   cost, per-frame H_pp (n x 36), g_p (n x 6), reduced S (D x D, undamped Schur complement), g_red (D),
 *   H_ss diagonal (D), g_s (D).
 * n = vc_num_frames: this rank's own frames on a sharded calibrator, its separator included, the ghost copy of the next rank's
 * separator excluded.  S and g_red are the all-reduced ones, separator columns included (D = vc_shared_dim). */
int vc_linearize(vc_calibrator* h, double* cost, double* Hpp, double* gp, double* S, double* g_red,
                 double* hss_diag, double* g_s);
int vc_shared_dim(vc_calibrator* h);
/* One LM pass at the current state with trust-region radius `radius` and the decision withheld (the state does not move; like
 * vc_linearize, every rank of a sharded calibrator calls it), then copies of what the pass left (any pointer may be NULL):
 *   cost at the linearisation point; the step of the shared parameters delta_s (D) and their damping lambda_s (D);
 *   the frames' damping (n x 9: pose 6, velocity 3 with the IMU; vision-only passes fill the first 6 of each row);
 *   the trial state the pass formed, in vc_get_frame / vc_get_camera layout: poses (n x 7, [q(4) t(3)]), velocities (n x 3),
 *   cameras (n_cams x 17: T_ck(7), then the intrinsics padded to 10), IMU parameters (15: g(2) b(6) sf(6) time offset(1)).
 * Velocities and IMU parameters are zero without inertial terms.  The frames' own steps are not stored by every form of the pass
 * (vision-only passes form them in registers): they are available only through the trial state.  On a sharded calibrator the
 * frames are this rank's, separators included, and delta_s holds the separators' steps at their columns.  Frame-indexed buffers
 * (frame_lam, poses, vels) hold n = vc_num_frames rows: the ghost copy of the next rank's separator is not read out. */
int vc_step_hold(vc_calibrator* h, double radius, double* cost, double* delta_s, double* slam, double* frame_lam, double* poses,
                 double* vels, double* cams, double* imus);
/* Runs exactly `iters` LM iterations of the real solver (complete solves back to back from the uploaded
 * initial state, the last one cut short); returns the number of iterations run (>= 0) or an error. */
int vc_run_iterations(vc_calibrator* h, int iters, int* jac_sweeps, int* res_sweeps);
/* Copies the device's accepted state -- where vc_run_iterations left it -- into what vc_get_camera, vc_get_frame, vc_get_biases,
 * vc_get_scale_factor, vc_get_gravity and vc_time_offset return (a solve does this itself when it ends; vc_run_iterations does not). */
int vc_download_state(vc_calibrator* h);
/* Per-tile reprojection residual sweep on the accepted state: cost (1/2 sum rho) and sum of squares */
int vc_evaluate(vc_calibrator* h, double* cost, double* sum_sq);
/* Times the dominant kernels with HIP events on the calibrator's stream: average ms per launch over reps */
int vc_time_kernels(vc_calibrator* h, int reps, double* jac_ms, double* res_ms);
/* In-loop kernel timing: with `on`, every launch group of every LM pass of the following solves is bracketed by HIP events
 * on the calibrator's stream (the real loop, decisions live -- not held back-to-back launches); vc_get_kernel_timing
 * returns, per group that ran, its name (';'-joined into names), the summed duration and the launch count. */
int vc_set_kernel_timing(vc_calibrator* h, int on);
/* Cross-stream hand-overs of the visual-inertial pass go through device flags.  A wait that runs into its bound is
 * never a silent change of results: the device withholds that pass's decision, the library reports it on stderr, resumes the
 * solve with event hand-overs (same iterates) and keeps them for this calibrator.  Returns how often that has happened. */
int vc_sync_timeouts(const vc_calibrator* h);
int vc_get_kernel_timing(vc_calibrator* h, char* names, int names_len, double* total_ms, long long* count, int max_entries);
/* Average ms per launch of each stage of one LM pass (Jacobian sweep, frame elimination, Schur partials,
 * reduced solve, trial sweep, decision), `reps` back-to-back launches each */
int vc_time_stages(vc_calibrator* h, int reps, double out[6]);
/* After vc_linearize with inertial terms active: weighted J^T J (33 x 33), J^T r (33), cost of each IMU block,
 * columns [frame j: pose 6, vel 3 | frame j-1: pose 6, vel 3 | g 2, b 6, sf 6, time offset 1].  Writes vc_num_imu_blocks blocks:
 * on a sharded calibrator, those this rank owns, the one that ends in the ghost frame included. */
int vc_get_imu_blocks(vc_calibrator* h, double* H, double* g, double* cost);
/* Current weight_sqrt_ factors W (9 x 9 per IMU block, row-major) with W W^T = (J Sigma J^T)^-1, after vc_linearize
 * with the weight update active (UpdateImuWeights, vicalibrator.h:723-799).  vc_num_imu_blocks blocks, as vc_get_imu_blocks. */
int vc_get_imu_weights(vc_calibrator* h, double* W);
/* ---- residual report: which corners, views, image regions and IMU blocks carry the error ------------------------------------
 * vc_report_compute runs two device sweeps at the current (accepted) state -- it uploads the problem first if it changed, like
 * vc_evaluate, without touching the solve's bookkeeping -- and keeps their results until the problem or the state changes; the other
 * entry points read slices of them.  Reading before a compute, or after an add_* / set_* / vc_clear / solve, is VC_ERR_BAD_ARG,
 * never stale data.  Not collective: a sharded rank reports its own frames (frame numbers are the rank's local ones).  Nothing is
 * allocated or launched for a calibrator that never asks.  bins_x / bins_y in [1, 32].  VC_ERR_RUNNING while a solve runs.
 * Which corners count: after an outlier stage (vc_set_remove_outliers) a corner is either dropped (vision-only calibration: no copy
 * of its residual block is left, it is not part of the problem any more) or kept with one copy fewer than the others
 * (visual-inertial calibration).  vc_get_camera_proj_rmse, the view rows and the error maps count every corner that still has a
 * copy, once each; dropped corners get a residual and a flag and enter no sum.  rmse of a camera = sqrt(sum sum_sq / (2 sum count))
 * over its views, which is what vc_get_camera_proj_rmse returns. */
int vc_report_compute(vc_calibrator* h, int bins_x, int bins_y);
/* Corners [first, first + n) in the order the caller added them (vc_add_observations / vc_add_observation_tiles call order, then the
 * order inside a call).  Any pointer may be NULL.  r: n x 2, (ru, rv) = projection - detection in pixels.  flags: bit 0 = dropped by
 * the outlier stage (residual still reported, at the same state), bit 1 = kept with one copy fewer. */
int vc_report_corners(vc_calibrator* h, long long first, long long n, double* r, int* frame, int* camera, unsigned char* flags);
long long vc_report_num_corners(vc_calibrator* h);   /* every corner the caller added, dropped ones included (< 0: a status) */
int vc_report_num_views(vc_calibrator* h);
/* One row per (frame, camera) that has corners, ordered by frame, then camera (any pointer may be NULL): count = corners still in the
 * problem, removed = corners the outlier stage marked (either kind), sum_sq = sum |r|^2 and max_err = max |r| over the corners still
 * in the problem, worst_corner = the index (as in vc_report_corners) of the corner that has the maximum, the lowest one on ties,
 * -1 in a view with no corner left. */
int vc_report_views(vc_calibrator* h, int* frame, int* camera, int* count, int* removed, double* sum_sq, double* max_err,
                    long long* worst_corner);
/* Error map of one camera: the image cut into bins_x x bins_y cells, a corner belongs to the cell of its DETECTED pixel (u, v):
 * ix = clamp(int(floor(u * bins_x / width)), 0, bins_x - 1), iy likewise with v, bins_y, height.  cells: bins_y x bins_x x 4 =
 * count, sum ru, sum rv, sum |r|^2 over the corners still in the problem (sums, so that the maps of several ranks add up).  Summed in
 * a fixed order: two reports of the same state give the same bits. */
int vc_report_error_map(vc_calibrator* h, int camera, double* cells);
/* IMU blocks of the report (vc_num_imu_blocks at the time of the compute; 0 without inertial terms in the stage), row s = the block
 * from frame s to frame s + 1: the 9 residuals as the cost sees them (times the block's current weight_sqrt_, rotation-only switch
 * applied: the block's cost is 1/2 x copies x CauchyLoss(100)(|whitened|^2)) and the 9 unweighted ones in the functor's order and
 * units (log of the pose difference: translation 3, rotation 3; velocity difference 3).  flags: bit 0 = the block's IMU sample range
 * is empty (rows are zero). */
int vc_report_num_imu_blocks(vc_calibrator* h);
int vc_report_imu(vc_calibrator* h, double* whitened /* x 9 */, double* unwhitened /* x 9 */, unsigned char* flags);
/* Times the sweeps of the last vc_report_compute with HIP events on the calibrator's stream, `reps` launches each: out_ms[0] the vision
 * sweep, [1] the error map's two passes, [2] the IMU sweep (the blocks' deltas + the residuals' tail; 0 without IMU blocks). */
int vc_time_report_sweeps(vc_calibrator* h, int reps, double out_ms[3]);
/* ---- held-out scoring: how well does the calibration predict views it has NOT seen? ----------------------------------------------
 * The hold-out set lives beside the problem, not in it: (frame, camera) groups of corners of held-out frames, numbered 0..n-1 in a
 * numbering of their own, that have no pose in the problem.  vc_holdout_compute freezes the cameras at the host state (what
 * vc_get_camera returns: after a solve, after vc_download_state, or on a calibrator that only had cameras added), refits the rig pose
 * of every held-out frame on the device -- one pose-only robust least-squares problem per frame, 1/2 sum SoftLOne(0.5)(|r|^2) over all
 * the frame's views jointly, Levenberg-Marquardt by the solver's own rules, first-order robustification (no Triggs correction) -- and
 * evaluates the residuals at the refitted poses.  It never uploads or invalidates the solve's problem and never touches vc_trace_len,
 * the iteration counters or the residual report; nothing is allocated or launched for a calibrator that never asks.  Tolerances are
 * those of vc_set_function_tolerance and vc_set_tolerances; max_iters <= 0 means 50, values above 200 mean 200.  Not collective: on
 * a sharded calibrator it is a local computation on whichever rank is asked.  VC_ERR_RUNNING while a solve runs.  The readers return
 * VC_ERR_BAD_ARG, never stale data, before a compute and after vc_holdout_add_tiles, vc_holdout_clear, vc_clear, vc_add_camera,
 * vc_fix_camera_intrinsics, a solve or anything else that changes what vc_get_camera returns.
 * Frame status: 0 converged, 1 max_iters (the pose is the last accepted one), 2 underdetermined (fewer than 4 corners over all of the
 * frame's views: not fitted, residuals evaluated at the seed), 3 no_seed (nothing evaluated: residuals and view sums are zero),
 * 4 failed (five steps in a row without a usable factorisation or model decrease, or a seed the cost is not finite at).  Only frames
 * of status 0 and 1 count as fitted. */
int vc_holdout_clear(vc_calibrator* h);
/* Same layout as vc_add_observation_tiles; tile_frame numbers the held-out frames; may be called repeatedly (appends; frame numbers
 * continue to mean the same frames; corners of one (frame, camera) given in several groups form one view, in order of arrival).  A
 * group of no corners still names its frame.  VC_ERR_BAD_ARG for a camera >= vc_num_cameras, a point id >= n_points or tile_off not
 * monotone; VC_ERR_TOO_MANY_POINTS beyond 32768 distinct points in the set, as for the problem (the set is then left unchanged). */
int vc_holdout_add_tiles(vc_calibrator* h, int n_tiles, const int* tile_frame, const int* tile_cam, const long long* tile_off /* n_tiles + 1 */,
                         const double* points, int n_points, const int* point_id, const double* p_c /* x 2 */);
/* seeds: n_frames x 7 T_wk, or NULL = seed every frame like vc_init_frame_poses_pnp does (camera 0 if it has >= 4 corners, else the
 * last camera that has; plain or RANSAC per vc_set_pnp_ransac); a frame no view of which gives a pose is no_seed. */
int vc_holdout_compute(vc_calibrator* h, const double* seeds, int max_iters);
int vc_holdout_num_frames(vc_calibrator* h);           /* 1 + the largest frame number named (< 0: a status) */
int vc_holdout_num_views(vc_calibrator* h);            /* (frame, camera) pairs that have corners */
long long vc_holdout_num_corners(vc_calibrator* h);
/* Per held-out frame (any pointer may be NULL): the refitted T_wk (the seed for status 2, identity for 3), status, LM iterations (steps
 * tried), cost = 1/2 sum rho at the seed and at the returned pose, behind = corners at camera-frame depth <= 0 at the returned pose
 * (such a corner enters no sum of the sweep that finds it there). */
int vc_holdout_frames(vc_calibrator* h, double* T_wk /* x 7 */, int* status, int* iterations, double* cost0, double* cost, int* behind);
/* One row per (frame, camera) that has corners, ordered by frame, then camera: count, sum |r|^2, max |r| and the corner that has it (index
 * as in vc_holdout_corners, the lowest on ties).  Views of flagged frames keep their rows; their status is the frame's. */
int vc_holdout_views(vc_calibrator* h, int* frame, int* camera, int* count, double* sum_sq, double* max_err, long long* worst_corner);
/* Corners [first, first + n) in the order the caller added them: r = n x 2 (ru, rv) = projection - detection in pixels. */
int vc_holdout_corners(vc_calibrator* h, long long first, long long n, double* r /* x 2 */, int* frame, int* camera);
/* Per camera sqrt(sum sum_sq / (2 sum count)) over its views of fitted frames (status 0 or 1) -- the convention of
 * vc_get_camera_proj_rmse -- and that corner count; 0 for a camera without such views. */
int vc_holdout_camera_rmse(vc_calibrator* h, double* rmse /* n_cameras */, long long* count /* n_cameras */);
/* Times the kernels of the last vc_holdout_compute with HIP events on the calibrator's stream, `reps` launches each, like
 * vc_time_report_sweeps: out_ms[0] the pose refit (from the seeds, every time), [1] the residual sweep. */
int vc_time_holdout(vc_calibrator* h, int reps, double out_ms[2]);
int vc_get_debug_stamps(vc_calibrator* h, long long out[32]);   /* shader-clock stamps of the last k_reduced (profiling aid) */
long long vc_num_observations(vc_calibrator* h);
int vc_num_tiles(vc_calibrator* h);

/* ---- image front-end, first slice -----------------------------------------------------------------------
 * Replaces, per image stream, the pair  calibu::ImageProcessing image_processing_[i](width, height)  +  calibu::ConicFinder
 * conic_finder_[i]  that VicalibTask owns (vicalib-task.h, constructed at vicalib-task.cc:115) and the two calls
 *     image_processing_[ii].Process(img->data(), img->Width(), img->Height(), img->Width());     vicalib-task.cc:264-267
 *     conic_finder_[ii].Find(image_processing_[ii]);                                             vicalib-task.cc:268
 * of AddImageMeasurements; the result is what the reference reads as conics[i].center (:296).  Parameters and defaults are the
 * ones VicalibTask sets (:116-122).  The image is an 8-bit greyscale HOST buffer (what HAL hands over); centres come back in
 * pixel coordinates (x, y), ordered by the smallest pixel index of their dot.  Grid matching (FindTarget, :274) is not part of
 * this slice.  No CPU fallback: vc_detector_create fails with VC_ERR_NO_DEVICE without a HIP device. */
typedef struct vc_detector vc_detector;
int vc_detector_create(int device, int width, int height, vc_detector** out);
void vc_detector_destroy(vc_detector* d);
int vc_detector_set_params(vc_detector* d, int black_on_white, double at_threshold, double at_window_ratio, double conic_min_area,
                           double conic_min_density, double conic_min_aspect);
/* The threshold window has half-width rad = (int)(width / at_window_ratio) and is clamped to the image.  The integral image is kept
 * modulo 2^32, which is exact only while a window's sum fits 32 bits: vc_detector_find / vc_detector_find_conics return
 * VC_ERR_UNSUPPORTED, before anything is uploaded, when  min(2 rad + 1, width) * min(2 rad + 1, height) * 255  does not (only
 * possible above 16.8 MP with a small at_window_ratio); the handle stays usable, set other parameters and call again.
 * A candidate whose conic fit is singular because no pixel of its box has a gradient (squared central difference >= 1) is not a dot:
 * it is neither returned nor counted in *n_found.  The limit of 4096 candidates per image (more: VC_ERR_UNSUPPORTED) is on the
 * candidates before that rule.  Fits that are rank-deficient with a non-zero matrix are not detected. */
/* centres: 2 x max_conics doubles; *n_found is the number of dots found (may exceed max_conics: the first max_conics are written).
 * A detector handle is single-threaded: one image at a time (its staging buffers and stream belong to the call in progress); use one
 * handle per thread. */
int vc_detector_find(vc_detector* d, const unsigned char* image, int pitch, double* centres, int max_conics, int* n_found);
/* The same with the rest of what calibu::Conic carries (vicalib-task.cc:270-277 hands the conics to TargetGridDot::FindTarget):
 * conics (nullable): 9 doubles per dot, the ellipse as a symmetric 3 x 3 matrix C with x^T C x = 0 on its edge, image coordinates
 * (pixel centres at integers), unit Frobenius norm, C[0][0] > 0 (calibu::Conic::C; Dual is its inverse, center what `centres` holds);
 * boxes (nullable): 4 ints per dot, the dot's bounding box x0, y0, x1, y1 inclusive (calibu::Conic::bbox). */
int vc_detector_find_conics(vc_detector* d, const unsigned char* image, int pitch, double* centres, double* conics, int* boxes, int max_conics,
                            int* n_found);
/* Second half of the front-end (vicalib-task.cc:274-277, calibu::TargetGridDot::FindTarget; vicalib-engine.cc:459-461,
 * calibu::MakePattern): which dot of the target is every detected conic?  Host code, no device needed (a few hundred dots per image).
 * vc_target_make_pattern: the large (1) / small (0) pattern of a rows x cols target from a seed (own generator: Calibu's is not in the
 * reference tree -- a printed Calibu target needs its own pattern).  vc_target_find: centres (2 per dot) and image ellipses (9 per dot,
 * as vc_detector_find_conics returns them) of one image -> dot_index (row * cols + col, or -1) per conic, the reference's
 * `ellipse_target_map`; *n_matched = 0 when no unambiguous placement exists (the reference then skips the frame).  Calibu's source
 * being absent, parity with FindTarget is unpinned; tests hold it to rendered views (tests/test_grid_cpu.py). */
int vc_target_make_pattern(int rows, int cols, unsigned seed, int* pattern);
int vc_target_find(const double* centres, const double* conics, int n, const int* pattern, int rows, int cols, int* dot_index, int* n_matched);

/* ---- using the calibration: undistortion on the device ----------------------------------------------------------------------------
 * What a caller of the reference does with cameras.xml through Calibu (Unproject, lookup-table rectification; tracker.cc:82-85 works with
 * a loaded model and K().inverse()): images and pixels of a calibrated SOURCE camera (any of the six models) mapped into an ideal pinhole
 * DESTINATION camera dst_linear = [fu fv u0 v0] of dst_w x dst_h pixels, rotated against the source by R_ds (row-major; maps source-camera
 * rays to destination-camera rays: pass a rectifying rotation for a stereo pair; NULL = identity).  Pixel centres are at integers, as in
 * the detector.  The handle builds its lookup table once (destination pixel -> source coordinate, fp32), owns a stream and pinned
 * staging buffers, and is single-threaded like a detector: one call in flight per handle.  No CPU fallback: VC_ERR_NO_DEVICE without a HIP
 * device.  VC_ERR_BAD_ARG: unknown model, wrong nparams, a size below 2 x 2 or above 8192, fill outside 0..255, an R_ds that is not a
 * rotation to 1e-9.
 * A destination pixel has NO source pixel -- it gets `fill` -- when its ray has z <= 0 in the source frame (any model but kb4), does not
 * project to finite coordinates, or lands outside [0, src_w - 1] x [0, src_h - 1] (closed to rounding: within 1e-9 px it is on the border). */
typedef struct vc_undistorter vc_undistorter;
int vc_undistorter_create(int device, int model, const double* params, int nparams, int src_w, int src_h, const double dst_linear[4], int dst_w,
                          int dst_h, const double R_ds[9], int fill, vc_undistorter** out);
/* the same for camera `camera` of a calibrator as vc_get_camera returns it (model, intrinsics and size), on the calibrator's device */
int vc_undistorter_create_for_camera(vc_calibrator* h, int camera, const double dst_linear[4], int dst_w, int dst_h, const double R_ds[9], int fill,
                                     vc_undistorter** out);
void vc_undistorter_destroy(vc_undistorter* u);
/* Destination intrinsics for identity rotation (host code, no device).  The source image's border -- its corners and 64 points inside every
 * edge -- is unprojected into the pinhole plane; samples without a pinhole image are dropped (fewer than 8 left: VC_ERR_NUMERIC).
 * alpha = 0: the axis-aligned rectangle between the innermost samples of the four edges fills the destination image, drawn in until every
 * destination pixel has a source pixel; alpha = 1: the bounding box of the samples fills it (every source pixel is kept); in between the
 * two rectangles are interpolated linearly.  alpha outside [0, 1] is VC_ERR_BAD_ARG. */
int vc_undistort_fit_linear(int model, const double* params, int nparams, int src_w, int src_h, int dst_w, int dst_h, double alpha, double dst_linear[4]);
/* n images, HOST buffers: image k starts at src + k * src_stride, its rows are src_pitch bytes apart (likewise dst); pitches may exceed the
 * widths, and a destination row's padding is not written.  Bilinear: x0 = min(floor(x), src_w - 2), ax = x - x0, likewise y; the value
 * (1 - ay) ((1 - ax) p00 + ax p01) + ay ((1 - ax) p10 + ax p11) in double precision, rounded half-up.  One upload, one launch, one
 * download and one synchronisation per call. */
int vc_undistort_images(vc_undistorter* u, int n, const unsigned char* src, int src_pitch, long long src_stride, unsigned char* dst, int dst_pitch,
                        long long dst_stride);
/* the same on DEVICE pointers, enqueued on the handle's stream (vc_undistort_stream, a hipStream_t) without synchronisation */
int vc_undistort_images_device(vc_undistorter* u, int n, const unsigned char* d_src, int src_pitch, long long src_stride, unsigned char* d_dst,
                               int dst_pitch, long long dst_stride);
void* vc_undistort_stream(vc_undistorter* u);
/* n distorted source pixels (x, y) -> pixels of the destination camera: the inverse the lookup table avoids.  Newton on the model's radial
 * profile r_d = f(r_u) (in theta for kb4) from r_u = r_d, analytic slope, at most 40 steps, stop at |f - r_d| <= 1e-14 (1 + r_d); then R_ds and
 * the pinhole projection.  valid (nullable) = 0 and a NaN pair: the iteration does not converge, leaves the positive range or meets a
 * non-positive slope (the pixel is beyond the model's image), the result is not finite, or the rotated ray has z <= 0. */
int vc_undistort_points(vc_undistorter* u, int n, const double* src_px /* n x 2 */, double* dst_px /* n x 2 */, unsigned char* valid /* n */);
/* the lookup table: map = dst_h x dst_w x 2 floats (x, y in the source image; a NaN pair where there is no source pixel), valid = dst_h x
 * dst_w bytes; either may be NULL */
int vc_undistort_get_map(vc_undistorter* u, float* map, unsigned char* valid);
int vc_undistort_get_linear(vc_undistorter* u, double dst_linear[4], int dst_size[2]);
/* HIP events on the handle's stream, `reps` launches each, like vc_time_report_sweeps: out_ms[0] the map build, [1] the remap of n_images
 * device-resident images, [2] 65536 points (a lattice over the source image). */
int vc_time_undistort(vc_undistorter* u, int n_images, int reps, double out_ms[3]);

/* ---- using the calibration of a PAIR: stereo rectification and the stereo consistency check ---------------------------------------
 * What the owner of a calibrated rig does with cameras.xml first: rotate both cameras into a common frame in which a point lies on the same
 * image row of both, with one pinhole camera dst_linear = [fu fv u0 v0] of dst_w x dst_h pixels for both sides, and see whether rows line
 * up and depth comes out in metres.  With p_c = R_ck p_k + t_ck, for cameras a and b: R = R_bk R_ak^T, t = t_bk - R t_ak (p_b = R p_a + t),
 * centre of b in a's frame c = -R^T t.
 * Rotations (row-major, source-camera rays -> rectified rays, what vc_undistorter_create takes as R_ds): e1 = c / |c|, negated if
 * e1 . xm < 0 with xm = x + R^T x the summed x axes (b to the left of a: the images stay upright); e2 = normalize(zm x e1) with
 * zm = z + R^T z the summed optical axes; e3 = e1 x e2; R_ds_a has the rows e1 e2 e3, R_ds_b = R_ds_a R^T.  The signed baseline is e1 . c
 * (negative when the sign flipped), and R_ds_b p_b = R_ds_a p_a - (baseline, 0, 0): same row, same depth Z, u_a - u_b = fu baseline / Z.
 * VC_ERR_NUMERIC: |c| < 1e-9.  VC_ERR_UNSUPPORTED: the baseline is closer to the images' vertical than to their horizontal
 * (|e1 . ym| > |e1 . xm|, ym = y + R^T y): column rectification is not provided.  VC_ERR_BAD_ARG: a pose that is not finite or whose
 * quaternion is not of unit length to 1e-6.  Host code, no device.  Any output pointer may be NULL. */
int vc_stereo_rectify_rotations(const double T_ck_a[7], const double T_ck_b[7], double R_ds_a[9], double R_ds_b[9], double* baseline);
/* One destination camera for both sides (host code, no device): the procedure of vc_undistort_fit_linear with each side's border samples
 * rotated by its R_ds (NULL = identity) before they enter the pinhole plane.  alpha = 1: the union of the two sides' bounding boxes fills
 * the destination image; alpha = 0: the intersection of the two inner rectangles, drawn in until every pixel of the destination border has
 * a source pixel on BOTH sides; in between the two rectangles are interpolated linearly.  VC_ERR_NUMERIC: an empty intersection, or fewer
 * than 8 samples of a side with a pinhole image. */
int vc_stereo_fit_linear(int model_a, const double* params_a, int nparams_a, int w_a, int h_a, const double R_ds_a[9], int model_b, const double* params_b,
                         int nparams_b, int w_b, int h_b, const double R_ds_b[9], int dst_w, int dst_h, double alpha, double dst_linear[4]);
/* Matched corners of two cameras in the layout of vc_add_observation_tiles (host code): for every frame that has a group of cam_a and a
 * group of cam_b, ordered by frame, the positions (indices into point_id / p_c) of the corners with equal point_id, ordered by point id;
 * of a point id given twice in one view the first position counts.  A frame with both cameras and no common corner keeps its (empty) row.
 * Two calls: with frame, frame_off, pos_a and pos_b NULL it only counts (*n_frames, *n_pairs); with arrays, *n_frames and *n_pairs hold
 * their capacities on entry (frame: n_frames, nullable; frame_off: n_frames + 1; pos_a, pos_b: n_pairs) and the counts on return;
 * VC_ERR_BAD_ARG if they do not fit. */
int vc_match_tiles(int n_tiles, const int* tile_frame, const int* tile_cam, const long long* tile_off /* n_tiles + 1 */, const int* point_id, int cam_a,
                   int cam_b, int* n_frames, long long* n_pairs, int* frame, long long* frame_off, long long* pos_a, long long* pos_b);
/* A rectifier: the rotations above, dst_linear (NULL = vc_stereo_fit_linear at alpha; alpha is not read otherwise) and one undistorter per
 * side, on `device`.  Single-threaded like an undistorter; no CPU fallback (VC_ERR_NO_DEVICE).  Argument errors are VC_ERR_BAD_ARG as in
 * vc_undistorter_create; they, the rotations' and the fit's statuses come before the device is looked for. */
typedef struct vc_rectifier vc_rectifier;
int vc_rectifier_create(int device, int model_a, const double* params_a, int nparams_a, int w_a, int h_a, const double T_ck_a[7], int model_b,
                        const double* params_b, int nparams_b, int w_b, int h_b, const double T_ck_b[7], const double dst_linear[4], int dst_w, int dst_h,
                        double alpha, int fill, vc_rectifier** out);
/* the same for cameras cam_a and cam_b of a calibrator as vc_get_camera returns them, on the calibrator's device */
int vc_rectifier_create_for_cameras(vc_calibrator* h, int cam_a, int cam_b, const double dst_linear[4], int dst_w, int dst_h, double alpha, int fill,
                                    vc_rectifier** out);
void vc_rectifier_destroy(vc_rectifier* r);
/* side 0 = a, 1 = b: that side's undistorter, BORROWED (never destroy it): its map, points, images and stream work as they do for any
 * undistorter.  NULL for another side. */
vc_undistorter* vc_rectifier_side(vc_rectifier* r, int side);
/* any pointer may be NULL.  T_ck_rect = (R_ds R_ck, R_ds t_ck): the rectified cameras' poses, which differ by a translation along x. */
int vc_rectifier_get(vc_rectifier* r, double R_ds_a[9], double R_ds_b[9], double dst_linear[4], int dst_size[2], double* baseline, double T_ck_rect_a[7],
                     double T_ck_rect_b[7]);
/* n image pairs, HOST buffers laid out as for vc_undistort_images: the same remap on the two sides' streams, both enqueued before either is
 * waited for, one synchronisation of each. */
int vc_rectify_pairs(vc_rectifier* r, int n, const unsigned char* src_a, int src_pitch_a, long long src_stride_a, const unsigned char* src_b, int src_pitch_b,
                     long long src_stride_b, unsigned char* dst_a, int dst_pitch_a, long long dst_stride_a, unsigned char* dst_b, int dst_pitch_b,
                     long long dst_stride_b);
/* The stereo consistency check, one device sweep over matched corner pairs: frame f holds pairs [frame_off[f], frame_off[f + 1]) of px_a /
 * px_b (n x 2 distorted pixels of the same target point in a and b; frame_off[0] = 0, at most 32768 pairs per frame) and of target (n x 3
 * target points in metres, or NULL).  A pair: both pixels through vc_undistort_points' arithmetic of their side -> (ua, va), (ub, vb);
 * dv = va - vb, d = ua - ub, Z = fu baseline / d, P = ((ua - u0) Z / fu, ((va + vb) / 2 - v0) Z / fv, Z) in the rectified frame of a.
 * pairs_out (n x 6, nullable): dv, d, P, (va + vb) / 2.  flags (n, nullable): 1 = INVALID pair -- an inversion failed or d baseline <= 0 --,
 * whose row is NaN and which enters no sum.  Per frame over its valid pairs (every array n_frames long and nullable): count, invalid,
 * sum dv, sum dv^2, max |dv| and the pair that has it (index into px_a, the lowest on ties, -1 without a valid pair), mean Z, and
 * rigid_rms: the RMS residual in metres of the best rigid fit (rotation + translation, NO scale: a wrong baseline shows) of the P onto
 * their target points; NaN without target or with fewer than 3 valid pairs.  A frame of no pairs has a zero row (worst -1, rms NaN).
 * Sums are formed in a fixed order: two runs, and a frame alone or among others, give the same bits.  n_frames = 0: VC_OK, no launch. */
int vc_rectify_check(vc_rectifier* r, int n_frames, const long long* frame_off /* n_frames + 1 */, const double* px_a, const double* px_b, const double* target,
                     double* pairs_out, unsigned char* flags, int* count, int* invalid, double* sum_dv, double* sum_dv2, double* max_abs_dv, long long* worst,
                     double* mean_z, double* rigid_rms);
/* HIP events on the rectifier's stream like vc_time_undistort: average ms of `reps` launches of the last vc_rectify_check's sweep on its
 * device-resident data (VC_ERR_BAD_ARG before a check). */
int vc_time_rectify_check(vc_rectifier* r, int reps, double* out_ms);

/* ---- comparing two calibrations of one camera in pixel space ----------------------------------------------------------------------
 * Did a recalibration change the camera, by how much, and where in the image?  Cameras A and B (any two of the six models) of the SAME
 * image size w x h, and a lattice of grid_x x grid_y samples: sample s = j grid_x + i sits at q = (i (w - 1) / (grid_x - 1),
 * j (h - 1) / (grid_y - 1)), at the normalised radius rho = |q - c| / |c| from the image centre c = ((w - 1) / 2, (h - 1) / 2).
 * Limits: 2 <= grid_x <= w, 2 <= grid_y <= h, grid_x grid_y <= 2^22.  The ray a of a sample is q through A's Newton inversion (the one of
 * the undistorter's points), scaled to unit length; b likewise through B.  The projection difference at a rotation R (row-major, A-camera
 * rays -> B-camera rays) is d = project(B, R a) - q.  flags: bit 0 A's inversion failed, bit 1 B's did, bit 2 the sample is INVALID -- an
 * inversion failed, (R a)_z <= 0 (unless B is kb4) or d is not finite --: its d is a NaN pair and it enters no sum.
 * The IMPLIED rotation is the one the extrinsics would absorb: over the fit set F (both inversions valid, rho <= fit_radius) it minimises
 * E(R) = sum |d(R)|^2.  Start: Horn's rotation of H = sum_F a b^T.  Then Gauss-Newton with R <- exp(w) R, rows J = -A [R a]x (A = the
 * 2 x 3 Jacobian of B's projection), w = -(sum J^T J)^-1 sum J^T d; a step that does not lower E is halved, up to 8 times; a sample of F
 * that is invalid at the current R is left out of that sweep and counted.  status 0: converged -- a Gauss-Newton step of |w| <= 1e-9 rad
 * (below 3.5e-7 px wherever f (1 + r_u^2) <= 3500), which is taken if it lowers E and is not halved; 1: max_iters reached (<= 0 means 20,
 * above 100 means 100); 2: no step lowered E, R is the last accepted one.  VC_ERR_NUMERIC: fewer than 3 samples in F, or a 3 x 3 system
 * without a positive pivot.
 * A comparer is single-threaded with a stream of its own; nothing is launched before the first run; no CPU fallback.  Argument errors are
 * VC_ERR_BAD_ARG and come before the device is looked for (VC_ERR_NO_DEVICE).  Every sum is formed in a fixed order that depends on the
 * lattice alone: two runs, and two handles, give the same bits.  Any output pointer may be NULL. */
typedef struct vc_comparer vc_comparer;
int vc_comparer_create(int device, int model_a, const double* params_a, int nparams_a, int model_b, const double* params_b, int nparams_b, int width,
                       int height, int grid_x, int grid_y, vc_comparer** out);
/* A = camera `camera` of a calibrator as vc_get_camera returns it (model, intrinsics and size), on the calibrator's device */
int vc_comparer_create_for_camera(vc_calibrator* h, int camera, int model_b, const double* params_b, int nparams_b, int grid_x, int grid_y, vc_comparer** out);
void vc_comparer_destroy(vc_comparer* c);
/* fit_radius > 0: the implied rotation is fitted, then the difference is taken at it.  fit_radius <= 0: no fit; R is R_ba (NULL = identity;
 * VC_ERR_BAD_ARG unless it is a rotation to 1e-9).  R_ba is not read when there is a fit.  One synchronisation per Gauss-Newton evaluation
 * and one for the difference sweep. */
int vc_compare_run(vc_comparer* c, double fit_radius, int max_iters, const double R_ba[9]);
/* The readers below return VC_ERR_BAD_ARG before a successful run.  cost0 = E(Horn's start), cost = E(R_ba); without a fit status,
 * iterations, the counts and the costs are zero. */
int vc_compare_get_fit(vc_comparer* c, double R_ba[9], int* status, int* iterations, int* n_fit, int* n_left_out, double* cost0, double* cost);
int vc_compare_get_map(vc_comparer* c, double* diff /* grid_y x grid_x x 2 */, unsigned char* flags /* grid_y x grid_x */);
/* over the valid samples: sum du, sum dv, sum |d|^2, and the largest |d| with its sample -- the lowest sample among those of the largest
 * |d|^2 = du du + dv dv (both products rounded), -1 without a valid sample */
int vc_compare_summary(vc_comparer* c, long long* count, long long* invalid, double* sum_du, double* sum_dv, double* sum_sq, double* max_err, long long* worst);
/* n_rings in [1, 64] arrays: ring k = min(int(rho n_rings), n_rings - 1).  The run bins 8 rings; another count is a rings-only sweep over the
 * stored d on the device (no inversion, no projection), kept until the next run or another count. */
int vc_compare_rings(vc_comparer* c, int n_rings, long long* count, long long* invalid, double* sum_sq, double* max_err);
/* Host code, no device: camera c >= 1 against camera 0 of rigs A and B, p_c = R_rel p_0 + t_rel from each rig's T_ck, centre of c in camera
 * 0's frame c_X = -R_rel_X^T t_rel_X.  R_0 and R_c (NULL = identity) are the implied rotations of cameras 0 and c.  out4 = the rotation
 * angle (rad) of R_rel_B^T R_c R_rel_A R_0^T and the distance |c_B - R_0 c_A|, then the same two with R_0 = R_c = I. */
int vc_compare_extrinsics(const double T_ck_a0[7], const double T_ck_ac[7], const double T_ck_b0[7], const double T_ck_bc[7], const double R_0[9],
                          const double R_c[9], double out4[4]);
/* HIP events on the comparer's stream like vc_time_undistort, after a run: average ms of `reps` launches of [0] the rays, [1] one fit sweep,
 * [2] the difference sweep, each with its reduction. */
int vc_time_compare(vc_comparer* c, int reps, double out_ms[3]);

/* ---- converting a calibrated camera to another camera model ---------------------------------------------------------------------------
 * A rig calibrated with one model handed to a consumer that speaks another, without calibrating again: source camera A (any of the six
 * models, image w x h), a target model m_b, and the comparer's lattice of grid_x x grid_y samples with its limits.  The ray a_s of sample s
 * is its pixel q_s through A's Newton inversion, scaled to unit length.  The fit set F holds the samples whose inversion succeeded and whose
 * rho <= fit_radius (>= 1: the whole image).  The result is the K_b of model m_b that minimises E(K_b) = sum over F of
 * |project(m_b, K_b, a_s) - q_s|^2.  No rotation, no change of extrinsics: the converted camera sees the same rays, T_ck stays valid.  A sample
 * of F with a_z <= 0 (unless m_b is kb4) or a d that is not finite is left out of a sweep and counted.
 * Levenberg-Marquardt on the host over device sweeps, one synchronisation per evaluation, with the rules of the calibration's own loop:
 * cost E / 2, initial radius 1e4, (H + D) delta = -g with D = clamp(diag H, 1e-6, 1e32) / radius; a step without a factorisation or a model
 * decrease halves the radius, five in a row end the fit as failed; a trial is accepted above a step quality of 1e-3.  status 0: converged --
 * |delta| <= 1e-10 (|x_free| + 1e-10) before a trial (the step is not taken), or |cost change| <= 1e-12 cost after an accepted step; 1:
 * max_iters trials (<= 0 means 50, above 200 means 200); 2: failed (the radius fell below 1e-32, or five invalid steps): K_b is the last
 * accepted point.  VC_ERR_NUMERIC: 2 n_fit is below the number of free parameters, or the first evaluation is not finite.
 * A converter is single-threaded with a stream of its own; nothing is launched before the first run; no CPU fallback.  Argument errors are
 * VC_ERR_BAD_ARG and come before the device is looked for (VC_ERR_NO_DEVICE).  Every sum is formed in a fixed order that depends on the
 * lattice alone: two runs, and two handles, give the same bits. */
typedef struct vc_converter vc_converter;
int vc_converter_create(int device, int model_a, const double* params_a, int nparams_a, int width, int height, int model_b, int grid_x, int grid_y,
                        vc_converter** out);
/* A = camera `camera` of a calibrator as vc_get_camera returns it (model, intrinsics and size), on the calibrator's device */
int vc_converter_create_for_camera(vc_calibrator* h, int camera, int model_b, int grid_x, int grid_y, vc_converter** out);
void vc_converter_destroy(vc_converter* c);
/* fit_radius > 0.  start: the nk_b start values, finite; NULL = [fu fv u0 v0] of A with the distortion parameters 0 (fov: w = 0.2, where the
 * reference starts it -- at w = 0 the model's derivative with respect to w is zero).  free_mask: bit k set = K_b[k] is free, 0 = all free,
 * no bit at or above nk_b; a fixed parameter stays at its start value. */
int vc_convert_run(vc_converter* c, double fit_radius, int max_iters, const double* start, unsigned int free_mask);
/* The last run: VC_ERR_BAD_ARG before a successful one; any pointer may be NULL.  params_b takes nk_b doubles.  iterations = trial points
 * evaluated; cost0 and cost = E / 2 at the start and at K_b, each from a values-only sweep of its own (the sums a comparer of A against that
 * camera gives); n_left_out, max_err and worst come from the sweep at K_b: the largest |d| over the fit set and its sample -- the lowest
 * among those of the largest |d|^2 = du du + dv dv (both products rounded). */
int vc_convert_get(vc_converter* c, double* params_b, int* nparams_b, int* status, int* iterations, int* n_fit, int* n_left_out, double* cost0, double* cost,
                   double* max_err, long long* worst);
/* A comparer of A against the result on the same lattice and device -- run at the identity rotation (fit_radius = 0, R_ba = NULL) it is the
 * conversion's residual per sample.  The caller destroys it. */
int vc_convert_comparer(vc_converter* c, vc_comparer** out);
/* HIP events on the converter's stream like vc_time_compare, after a run: average ms of `reps` launches of [0] the rays, [1] one
 * linearisation, [2] one cost sweep, each with its reduction. */
int vc_time_convert(vc_converter* c, int reps, double out_ms[3]);

/* ---- mapping the projection uncertainty of a calibrated camera ------------------------------------------------------------------------
 * How far can this calibration be trusted, and where in the image?  Camera A (any of the six models, intrinsics K -- nk of them --, image
 * w x h), the comparer's lattice of grid_x x grid_y samples with its limits, a covariance Cov of K (nk x nk, row-major), a noise scale
 * sigma_px > 0 and a fit_radius.  The ray a_s of sample s is its pixel q_s through A's Newton inversion, scaled to unit length.  B_s (2 x nk,
 * with respect to K) and A_s (2 x 3, with respect to the ray) are the Jacobian blocks of A's projection at a_s; Jw_s = -A_s [a_s]x is the
 * comparer's rotation row at R = I.  The fit set F: inversion valid, rho <= fit_radius, a_z > 0 unless the model is kb4.  Over F,
 * G = sum Jw^T Jw (3 x 3), C = sum Jw^T B (3 x nk) and M = -G^-1 C, in rad per unit of each parameter: a change dK moves sample s by
 * B_s dK, the rotation that best absorbs it over F -- the one the extrinsics, or the pose of whoever uses the camera, would take up -- is
 * w = M dK, and what is left is J_s dK with J_s = B_s + Jw_s M.  fit_radius <= 0: no compensation, M = 0 and J_s = B_s.
 * The map: Sigma_s = sigma_px^2 J_s Cov J_s^T, a symmetric 2 x 2 stored as (s_uu, s_uv, s_vv) in px^2.  var_s = s_uu + s_vv is the
 * expected squared shift of the sample; lam_s = (var_s + sqrt((s_uu - s_vv)^2 + 4 s_uv^2)) / 2, clamped at 0, is the variance along the
 * worst direction.  Every valid sample gets a value, in F or not.  flags: bit 0 A's inversion failed, bit 2 the sample is INVALID -- the
 * inversion failed, a_z <= 0 (unless kb4) or Sigma is not finite --: its triple is NaN and it enters no sum.  Cov is multiplied by
 * sigma_px^2 before it enters the sweep: doubling sigma_px quadruples every output bit for bit.
 * What the map does NOT say: it is the intrinsics' share after a rotation, for one camera on its own -- the baseline and the relative pose
 * of a stereo pair carry an uncertainty of their own that is not in it --, and like any covariance it assumes the noise model of the solve.
 * VC_ERR_NUMERIC: fewer than 3 samples in F, or a G without a positive pivot.  A handle is single-threaded with a stream of its own;
 * nothing is launched before the first run; no CPU fallback.  Argument errors are VC_ERR_BAD_ARG and come before the device is looked for
 * (VC_ERR_NO_DEVICE).  Every sum is formed in a fixed order that depends on the lattice alone: two runs, and two handles, give the same
 * bits.  Any output pointer may be NULL. */
typedef struct vc_uncertainty vc_uncertainty;
int vc_uncertainty_create(int device, int model, const double* params, int nparams, int width, int height, int grid_x, int grid_y, vc_uncertainty** out);
/* A = camera `camera` of a calibrator as vc_get_camera returns it (model, intrinsics and size), on the calibrator's device, with the
 * camera's params block of vc_get_solution_covariance at the current state kept as the handle's covariance: collective on a sharded
 * calibrator like that call, whose status is handed on (VC_ERR_NUMERIC included).  VC_ERR_BAD_ARG with fixed intrinsics: no block then. */
int vc_uncertainty_create_for_camera(vc_calibrator* h, int camera, int grid_x, int grid_y, vc_uncertainty** out);
void vc_uncertainty_destroy(vc_uncertainty* u);
/* cov: nk x nk, NULL = the calibrator's (VC_ERR_BAD_ARG on a handle without one).  VC_ERR_BAD_ARG: an entry of cov that is not finite,
 * cov not symmetric to 1e-12 max |diag|, a negative diagonal entry, sigma_px not > 0 and finite, fit_radius not finite.  The rays are
 * computed once per handle; another fit_radius redoes only the sweep of G and C.  A refused run leaves nothing to read. */
int vc_uncertainty_run(vc_uncertainty* u, const double* cov, double sigma_px, double fit_radius);
/* The readers below return VC_ERR_BAD_ARG before a successful run.  Without compensation M, G and n_fit are zero. */
int vc_uncertainty_get_fit(vc_uncertainty* u, double* M /* 3 x nk */, double* G /* 3 x 3 */, int* n_fit);
int vc_uncertainty_get_map(vc_uncertainty* u, double* sigma /* grid_y x grid_x x 3 */, unsigned char* flags /* grid_y x grid_x */);
/* over the valid samples: sum var, and the largest lam with its sample -- the lowest among equal ones, -1 (and max_lam 0) without a valid sample */
int vc_uncertainty_summary(vc_uncertainty* u, long long* count, long long* invalid, double* sum_var, double* max_lam, long long* worst);
/* n_rings in [1, 64] arrays, the comparer's rings.  The run bins 8; another count is a rings-only sweep over the stored triples on the
 * device, kept until the next run or another count.  max_lam of a ring without a valid sample is 0. */
int vc_uncertainty_rings(vc_uncertainty* u, int n_rings, long long* count, long long* invalid, double* sum_var, double* max_lam);
/* HIP events on the handle's stream like vc_time_compare, after a run: average ms of `reps` launches of [0] the rays, [1] the sweep of G
 * and C, [2] the map sweep, each with its reduction. */
int vc_time_uncertainty(vc_uncertainty* u, int reps, double out_ms[3]);

/* ---- mapping the row and depth uncertainty of a calibrated stereo pair ---------------------------------------------------------------
 * By how many pixels will the rows of the rectified images disagree, and where?  How wrong is a depth of 2 m?  Cameras A and B (model,
 * intrinsics, size, T_ck), the rectified frames of vc_stereo_rectify_rotations and a destination pinhole dst_linear of dst_w x dst_h that
 * is held FIXED (NULL = vc_stereo_fit_linear at alpha, as vc_rectifier_create).  A sample is a point (x, y) of the comparer's lattice of
 * grid_x x grid_y points over the rectified image of A together with a depth Z > 0: the point ((x - u0) Z / fu, (y - v0) Z / fv, Z) of A's
 * rectified frame, seen by the two cameras at pixels p_a and p_b.  A user who holds a slightly different calibration pushes those pixels
 * through the rectifier's arithmetic (vc_rectify_check) and gets the row misalignment dv, the disparity d and the depth Z off by a shift that
 * is linear in the calibration's error; with the covariance of the calibration that shift has the variances (var_dv, var_d, var_Z) in
 * px^2, px^2 and m^2, which is what the map stores per sample and depth.  cov is the joint covariance of the pair in the layout a
 * two-camera rig's vc_get_solution_covariance has -- q_a (4) p_a (3) K_a q_b (4) p_b (3) K_b, n = 14 + nk_a + nk_b, row-major --, multiplied
 * by sigma_px^2 before it enters the sweep: doubling sigma_px quadruples every output bit for bit.  The pose part goes through W, the 7 x 12
 * derivative of (w_a, w_b, baseline) -- R_ds moving as exp([w]x) R_ds -- with respect to (w_ck_a, dp_a, w_ck_b, dp_b), the poses moving as
 * q <- q * exp(w_ck), p <- p + dp (vc_stereo_pose_jacobian; host code, the statuses of vc_stereo_rectify_rotations).
 * flags: bit 0 the point is not seen by A (behind the camera unless kb4, or its pixel outside [0, w - 1] x [0, h - 1]), bit 1 the same for
 * B, bit 2 the sample is INVALID -- either of the two, or a variance that is not finite --: its triple is NaN and it enters no sum.
 * What the map does NOT say: dst_linear is held fixed (a user who refits it moves every pixel by more), the two images' noise and the
 * matching error are not in it, and like any covariance it assumes the noise model of the solve.
 * A run takes 1 to 8 depths, each > 0 and finite; the planes are swept one after the other on the handle's stream with one
 * synchronisation per run, and a plane's bits do not depend on the planes beside it.  A handle is single-threaded with a stream of its
 * own; nothing is launched before the first run; no CPU fallback.  Argument errors are VC_ERR_BAD_ARG; they, the rotations' and the fit's
 * statuses come before the device is looked for (VC_ERR_NO_DEVICE).  Every sum is formed in a fixed order that depends on the lattice
 * alone: two runs, and two handles, give the same bits.  Any output pointer may be NULL. */
typedef struct vc_stereo_uncertainty vc_stereo_uncertainty;
int vc_stereo_pose_jacobian(const double T_ck_a[7], const double T_ck_b[7], double W[84]);
int vc_stereo_uncertainty_create(int device, int model_a, const double* params_a, int nparams_a, int w_a, int h_a, const double T_ck_a[7], int model_b,
                                 const double* params_b, int nparams_b, int w_b, int h_b, const double T_ck_b[7], const double dst_linear[4], int dst_w, int dst_h,
                                 double alpha, int grid_x, int grid_y, vc_stereo_uncertainty** out);
/* the same for cameras cam_a and cam_b of a calibrator as vc_get_camera returns them, on the calibrator's device, with the pair's rows and
 * columns of vc_get_solution_covariance at the current state kept as the handle's covariance: collective on a sharded calibrator like that
 * call, whose status is handed on (VC_ERR_NUMERIC included).  VC_ERR_BAD_ARG with fixed intrinsics: no intrinsics blocks then. */
int vc_stereo_uncertainty_create_for_cameras(vc_calibrator* h, int cam_a, int cam_b, const double dst_linear[4], int dst_w, int dst_h, double alpha, int grid_x,
                                             int grid_y, vc_stereo_uncertainty** out);
void vc_stereo_uncertainty_destroy(vc_stereo_uncertainty* u);
/* the handle's geometry: the rectifying rotations, the destination pinhole, the signed baseline and W */
int vc_stereo_uncertainty_get(vc_stereo_uncertainty* u, double R_ds_a[9], double R_ds_b[9], double dst_linear[4], double* baseline, double W[84]);
/* cov: n x n, NULL = the calibrator's (VC_ERR_BAD_ARG on a handle without one).  VC_ERR_BAD_ARG: an entry of cov that is not finite, cov
 * not symmetric to 1e-12 max |diag|, a negative diagonal entry, sigma_px not > 0 and finite, n_depths outside [1, 8], a depth that is not
 * > 0 and finite.  A refused run leaves nothing to read. */
int vc_stereo_uncertainty_run(vc_stereo_uncertainty* u, const double* cov, double sigma_px, const double* depths, int n_depths);
/* The readers below return VC_ERR_BAD_ARG before a successful run. */
int vc_stereo_uncertainty_get_map(vc_stereo_uncertainty* u, double* var /* n_depths x grid_y x grid_x x 3 */, unsigned char* flags /* n_depths x grid_y x grid_x */);
/* of depth plane `plane` of the last run, over its valid samples: the three sums of variances and the largest var_dv with its sample -- the
 * lowest among equal ones, -1 (and max_var_dv 0) without a valid sample */
int vc_stereo_uncertainty_summary(vc_stereo_uncertainty* u, int plane, long long* count, long long* invalid, double* sum_var_dv, double* sum_var_d, double* sum_var_z,
                                  double* max_var_dv, long long* worst);
/* sigma_px^2 W Cov W^T of the last run, its diagonal: the variances of w_a (3, rad^2), of w_b (3) and of the baseline (m^2) */
int vc_stereo_uncertainty_get_pose_sigma(vc_stereo_uncertainty* u, double var[7]);
/* HIP events on the handle's stream like vc_time_compare, after a run: average ms of `reps` launches of [0] the two side sweeps of one depth
 * plane, [1] the map sweep with its reduction. */
int vc_time_stereo_uncertainty(vc_stereo_uncertainty* u, int reps, double out_ms[2]);

/* ---- view selection: which frames carry the information? -----------------------------------------------------------------------------
 * Greedy D-optimal selection over candidate frames of a rig of up to 8 cameras.  Inputs are where the target was seen, not what was
 * measured: per camera a model, intrinsics, T_ck and the solver's flags (1 rotation free, 2 translation free, 4 intrinsics free); per
 * frame a rig pose T_wk and (frame, camera) groups of target points.  Information is taken at unit pixel noise without a robust loss.
 * The shared columns are the solver's: per camera [w_ck (3)][t_ck (3)][K (nk)] as far as free, cameras in order, D columns in all.
 * LIMIT: D <= 64; a rig beyond it is refused with VC_ERR_UNSUPPORTED.
 * Frame information, the frame's pose marginalised: with J = [J_f (2n x 6) | J_s (2n x D)] over the frame's corners (the columns the
 * solver forms), I_f = J_s^T J_s - J_s^T J_f (J_f^T J_f)^-1 J_f^T J_s.  A corner at camera depth <= 0 (any model but kb4) enters no sum
 * and is counted as `behind`; it does not count as a corner.  Frame status: 0 usable; 1 underdetermined -- fewer than 4 corners over all
 * views, or the Cholesky of J_f^T J_f meets a pivot <= 1e-12 x its largest diagonal entry --: I_f = 0, never selected; 2 some corner lay
 * behind a camera, still usable.  Scaling: s_j = 1 / sqrt(sum_f I_f[j][j]) over usable frames (1 where the sum is 0) and I~_f =
 * diag(s) I_f diag(s); differences of log-determinants do not depend on it.
 * Selection: S_0 = prior I + sum over the start set of I~_f.  Round k gives every usable frame not yet in the set gain_k(f) =
 * logdet(S_{k-1} + I~_f) - logdet(S_{k-1}), picks the largest (the lowest frame on exactly equal gains) and adds it.  It ends after k
 * picks, when no candidate is left, or when the best gain is <= 0.  cum_k = logdet(S_k) - logdet(S_0); total = logdet(S_0 + sum of I~_f
 * over every usable frame outside the start set) - logdet(S_0): cum_k / total is the share of the attainable information the first k
 * views carry.  All rounds run on the device without a host synchronisation between them; two runs on the same input give the same bits.
 * Accuracy (tests/select_cases.py): the device agrees with a float64 numpy reference to 16 x that reference's own distance from its
 * long-double evaluation.  A handle is single-threaded with a stream of its own; nothing is allocated on the device before the first run;
 * no CPU fallback (VC_ERR_NO_DEVICE).  Argument errors are VC_ERR_BAD_ARG and leave the handle unchanged.  The readers return
 * VC_ERR_BAD_ARG, never stale data, before a run and after vc_select_add_tiles or vc_select_set_poses.  Any output pointer may be NULL. */
typedef struct vc_selector vc_selector;
int vc_selector_create(int device, int n_cameras, const int* model, const double* params /* x 10, padded */, const int* nparams,
                       const double* T_ck /* x 7 */, const int* cam_flags, vc_selector** out);
/* The cameras at the host state (what vc_get_camera returns), the calibrator's flags (camera 0 pinned unless the inertial terms are
 * active, vc_fix_camera_intrinsics), its frames' poses and its observation tiles (corners the outlier pass removed are left out), on
 * the calibrator's device.  VC_ERR_RUNNING while a solve runs. */
int vc_selector_create_for_calibrator(vc_calibrator* h, vc_selector** out);
void vc_selector_destroy(vc_selector* s);
/* Same layout and rules as vc_holdout_add_tiles without the pixel column: tile_frame numbers the candidate frames; appends; the corners
 * of one (frame, camera) given in several groups form one view, in order of arrival.  VC_ERR_BAD_ARG for a camera >= n_cameras, a point
 * id >= n_points or tile_off not monotone. */
int vc_select_add_tiles(vc_selector* s, int n_tiles, const int* tile_frame, const int* tile_cam, const long long* tile_off /* n_tiles + 1 */,
                        const double* points, int n_points, const int* point_id);
int vc_select_set_poses(vc_selector* s, const double* T_wk /* n_frames x 7 */, int n_frames);
/* VC_ERR_BAD_ARG: k < 1, a start-set frame out of range or repeated, prior not finite or <= 0 (1e-6 is the tools' default), a tile that
 * names a frame without a pose. */
int vc_select_run(vc_selector* s, int k, const int* start_set, int n_start, double prior);
int vc_select_get(vc_selector* s, int* n_picked, int* order /* k */, double* gain /* k */, double* cum /* k */, double* total);
int vc_select_frames(vc_selector* s, int* status, int* corners, int* behind);      /* n_frames each */
int vc_select_frame_information(vc_selector* s, int frame, double* I /* D x D, unscaled */, double* scale /* D */);
/* the gains of all candidates in the last round that ran; -1 for frames that were selected before it, in the start set, or unusable */
int vc_select_last_gains(vc_selector* s, double* gains /* n_frames */);
int vc_select_dim(vc_selector* s);                      /* D (< 0: a status) */
/* HIP events on the handle's stream, after a run: average ms of `reps` launches of [0] the information sweep, [1] one gain round at
 * the last state over every candidate left, [2] one pick (it stores nothing). */
int vc_time_select(vc_selector* s, int reps, double out_ms[3]);

/* ---- registering a depth image into another camera of the rig ------------------------------------------------------------------------
 * What the owner of a rig with a depth sensor does with cameras.xml first: put the depth image into the colour camera's pixels, or the
 * colour image into the depth camera's.  The SOURCE camera S is the depth camera, the DESTINATION camera D the other one; each has a
 * model (any of the six), params and a size from 2 x 2 to 8192 x 8192, checked as by vc_undistorter_create.  Poses T_ck_s, T_ck_d as
 * vc_get_camera returns them; with p_c = R_ck p_k + t_ck: R = R_dk R_sk^T, t = t_dk - R t_sk, p_d = R p_s + t (the rectifier's pair
 * relation).  A pose that is not finite or whose quaternion is not of unit length to 1e-6 is VC_ERR_BAD_ARG.
 * Depth image: uint16, rows `pitch` bytes apart (even; the buffer 2-byte aligned).  0 = no measurement; v = v * unit_src metres;
 * unit_src > 0, unit_dst > 0, both finite.  kind 0 (Z): the value is the distance along S's optical axis; kind 1 (range): along the
 * pixel's ray.  Pixel centres are at integers.
 * The ray r of a source position (u, v) is the Newton inversion of vc_undistort_points.  The centre of pixel (i, j) with measured distance
 * m lies at p_s = r (m / r_z) under kind Z (needs r_z > 0), p_s = r m / |r| under kind range; its value in D is m_d = (p_d)_z under kind Z,
 * |p_d| under kind range, and w = floor(m_d / unit_dst + 0.5).
 * A source pixel is dropped by the FIRST of these rules that applies; each has a counter:
 *   0  value 0
 *   1  no ray: the inversion failed, or r_z <= 0 under kind Z
 *   2  (p_d)_z <= 0 unless D is kb4 (the undistorter's rule), or the projection is not finite
 *   3  lands outside [0, w_d - 1] x [0, h_d - 1]
 *   4  w outside 1..65535
 *   5  footprint larger than 8 pixels in x or y (footprint mode only)
 *   6  candidates that reached the depth test (not a drop)
 *   7  destination pixels filled (not a drop)
 * splat 0 (nearest): the candidate lands on (floor(q_x + 0.5), floor(q_y + 0.5)), q = the projection of p_d into D.
 * splat 1 (footprint), for a D finer than S: the positions (i - 0.5, j - 0.5) and (i + 0.5, j + 0.5) are unprojected, placed at the
 * pixel's own measured distance m by the formula of the centre, transformed and projected to qa, qb; either corner failing rule 1 or 2
 * drops the pixel under that rule.  The rectangle x0 = floor(min(qa_x, qb_x) + 0.5) .. x1 = floor(max(qa_x, qb_x) + 0.5), likewise y:
 * empty after clipping to the image is rule 3, more than 8 wide or high before clipping rule 5; the candidate lands on every pixel of the
 * clipped rectangle.  The value w is always that of the pixel centre: the mode changes where a value lands, never the value.
 * Depth test: a candidate's key is (w << 32) | (j w_s + i); a destination pixel takes the SMALLEST key that landed on it -- the nearest
 * surface, among equal values the lowest source index.  Where nothing landed the depth is 0 and the index -1.  A minimum does not depend
 * on the order of arrival: two runs, and an image alone or in a batch, give the same bytes.
 * Colour into depth geometry: D's 8-bit image taken into S's pixels.  Source pixel (i, j) is VISIBLE when its centre passes rules 0-2, its centre
 * projection q lies in D's image under the undistorter's border rule (within 1e-9 px it is on the border), and the pixel
 * (floor(q_x + 0.5), floor(q_y + 0.5)) of the depth test just run (in the handle's splat mode) holds a value w_win with
 * w <= w_win + occl_tol (occl_tol >= 0, in units of unit_dst).  A visible pixel gets D's image at q by the bilinear rule of
 * vc_undistort_images (double precision, rounded half-up), every other pixel `fill`.
 * The ray tables (every pixel centre and every node of the corner lattice) are built once, at create.  A handle is single-threaded, with
 * a stream and pinned staging of its own that grow with the batch size.  Argument errors are VC_ERR_BAD_ARG and come before the device is
 * looked for; no CPU fallback (VC_ERR_NO_DEVICE).  n = 0 is VC_OK without a launch; n <= 65535. */
typedef struct vc_registrar vc_registrar;
int vc_registrar_create(int device, int model_s, const double* params_s, int nparams_s, int w_s, int h_s, const double T_ck_s[7], int model_d,
                        const double* params_d, int nparams_d, int w_d, int h_d, const double T_ck_d[7], double unit_src, double unit_dst, int kind,
                        int splat, vc_registrar** out);
/* the same for cameras cam_s and cam_d of a calibrator as vc_get_camera returns them, on the calibrator's device */
int vc_registrar_create_for_cameras(vc_calibrator* h, int cam_s, int cam_d, double unit_src, double unit_dst, int kind, int splat, vc_registrar** out);
void vc_registrar_destroy(vc_registrar* r);
/* R (row-major), t, both sizes (w, h), units = [unit_src, unit_dst], kind, splat; any pointer may be NULL */
int vc_register_get(vc_registrar* r, double R[9], double t[3], int size_s[2], int size_d[2], double units[2], int* kind, int* splat);
/* n depth images of S, HOST buffers (image k at src + k * src_stride BYTES, rows src_pitch bytes apart; likewise dst) -> n depth images
 * in D's pixels; a destination row's padding is not written.  index (nullable): n x h_d x w_d int32, the source index j w_s + i that won,
 * -1 where nothing landed.  counters (nullable): n x 8, the table above.  One upload, the launches (clear, scatter, resolve), one
 * download and one synchronisation per call. */
int vc_register_depth(vc_registrar* r, int n, const unsigned short* src, int src_pitch, long long src_stride, unsigned short* dst, int dst_pitch,
                      long long dst_stride, int* index, long long* counters);
/* the same on DEVICE pointers, enqueued on the handle's stream (vc_register_stream, a hipStream_t) without synchronisation; a batch larger
 * than any before first waits for the stream and grows the key buffer */
int vc_register_depth_device(vc_registrar* r, int n, const unsigned short* d_src, int src_pitch, long long src_stride, unsigned short* d_dst,
                             int dst_pitch, long long dst_stride, int* d_index, long long* d_counters);
void* vc_register_stream(vc_registrar* r);
/* n depth images of S and n 8-bit images of D (HOST buffers) -> n 8-bit images of w_s x h_s: the depth test, then the gather.  mask
 * (nullable): n x h_s x w_s bytes, 1 = visible.  VC_ERR_BAD_ARG: occl_tol < 0 or not finite, fill outside 0..255. */
int vc_register_color(vc_registrar* r, int n, const unsigned short* depth, int depth_pitch, long long depth_stride, const unsigned char* color,
                      int color_pitch, long long color_stride, double occl_tol, int fill, unsigned char* out, int out_pitch, long long out_stride,
                      unsigned char* mask);
/* The continuous face: n rows (u, v, value) at arbitrary sub-pixel positions of S -- the Newton inversion runs per point, the tables are
 * not read -- -> n rows (q_x, q_y, m_d / unit_dst) before any rounding.  valid (nullable) = 0 and a NaN row: rule 1 or 2, or a value that
 * is not positive and finite. */
int vc_register_points(vc_registrar* r, int n, const double* in /* n x 3 */, double* out /* n x 3 */, unsigned char* valid /* n */);
/* HIP events on the handle's stream, `reps` launches each: out_ms[0] the table build, [1] clear + scatter + resolve of n_images
 * device-resident images (a slanted surface of 1000..2499 counts), [2] the gather, [3] 65536 points. */
int vc_time_register(vc_registrar* r, int n_images, int reps, double out_ms[4]);

/* ---- calibrating a depth camera's range error against the target ---------------------------------------------------------------------
 * A calibration run holds what is needed to measure the range error of a depth sensor directly: every frame has a pose T_wk, the depth
 * camera S has intrinsics and T_ck, and the target is a plane at z_w = 0 of known extent.  For every depth pixel that looks at the board
 * the distance the sensor should have reported is known; compared with what it did report, over all frames and pixels, that gives the
 * error as a function of value and image position, and from it a correction to apply before vc_register_depth.
 * The handle holds S (any of the six models, params, a size from 2 x 2 to 8192 x 8192, T_ck; checked as by vc_registrar_create), unit
 * (metres per count) and kind (0 Z, 1 range) as the registrar defines them, the board rectangle rect = [x0, y0, x1, y1] in the target plane
 * (metres; x0 < x1, y0 < y1, finite), bins_x, bins_y in 1..32, v_ref > 0 (counts: a typical value of the working range, which only
 * centres the arithmetic), min_cos in (0, 1] and max_dev > 0 (counts).
 * Geometry.  With p_c = R_ck p_k + t_ck and p_w = R_wk p_k + t_wk: R_wc = R_wk R_ck^T, c_w = t_wk - R_wc t_ck.  For pixel (i, j) of a
 * frame with value v: the ray r is the registrar's (Newton inversion of vc_undistort_points at the pixel centre; r_z > 0 required under
 * kind Z); d_w = R_wc r; s = -c_w.z / d_w.z; hit = c_w + s d_w; the expected distance e = s r_z (kind Z) or s |r| (kind range); in
 * counts y = e / unit.
 * A pixel is dropped by the FIRST of these rules that applies; each is counted per frame:
 *   0  v == 0
 *   1  no ray (the registrar's rule 1)
 *   2  s not finite or s <= 0: the plane is not in front along the ray
 *   3  hit outside rect (closed)
 *   4  |d_w.z| < min_cos |d_w|: grazing incidence
 *   5  y outside [1, 65535]
 *   6  |y - v| > max_dev: the gate (an occluder, a hand, a multipath blunder)
 *   7  pixels used (not a drop)
 * A used pixel adds, with x = (v - v_ref) / v_ref and d = y - v, to the nine sums [1, x, x^2, x^3, x^4, d, d x, d x^2, d^2] of its image
 * cell (report_cell(i, bins_x, w), report_cell(j, bins_y, h)), the binning of the report's error maps; cell index cy * bins_x + cx.  The
 * handle keeps bins_x * bins_y * 9 running sums, 8 running counters and a frame count over everything added since create or clear.  The
 * order in which a pixel's terms enter a cell's sums depends on the image size, the bins and the order of the frames only: a batch of 8,
 * 3 + 5 and eight single calls give the same bits, as do two runs and two handles.
 * Fit, from the sums alone, on the host.  Stage 1: P(x) = c0 + c1 x + c2 x^2 of degree g in {0, 1, 2} fitted to d by least squares over
 * the totals (VC_ERR_NUMERIC without a pixel or without a positive pivot).  Stage 2, per cell: a + b x fitted to the remainder d - P(x),
 * whose sums follow from the nine.  status 0: n >= min_count and the variance of x in the cell >= min_spread^2 -- a and b fitted;
 * 1: enough pixels but too little spread -- a alone, b = 0; 2: too few pixels -- a = b = 0.  rms[3] in counts, from the sums: raw
 * (sqrt(S_dd / n)), after stage 1, after stage 2.
 * Correction of a value v != 0 at pixel (i, j): delta = P(x) + A + B x, v' = floor(v + delta + 0.5); a v' outside 1..65535 becomes 0 and
 * is counted.  interp 0: (A, B) are the pixel's own cell's (a, b); interp 1: bilinear between cell centres, fx = (i + 0.5) bins_x / w - 0.5
 * clamped to [0, bins_x - 1], k0 = floor(fx), k1 = min(k0 + 1, bins_x - 1), likewise in y.
 * Images are HOST buffers under the registrar's pitch / stride / alignment rules.  A handle is single-threaded, with a stream and pinned
 * staging of its own.  Argument errors are VC_ERR_BAD_ARG and come before the device is looked for; no CPU fallback (VC_ERR_NO_DEVICE).
 * n = 0 is VC_OK without a launch; n <= 65535. */
typedef struct vc_depthcal vc_depthcal;
int vc_depthcal_create(int device, int model, const double* params, int nparams, int w, int h, const double T_ck[7], double unit, int kind,
                       const double rect[4], int bins_x, int bins_y, double v_ref, double min_cos, double max_dev, vc_depthcal** out);
/* the same for camera cam of a calibrator as vc_get_camera returns it, on the calibrator's device */
int vc_depthcal_create_for_camera(vc_calibrator* h, int cam, double unit, int kind, const double rect[4], int bins_x, int bins_y, double v_ref,
                                  double min_cos, double max_dev, vc_depthcal** out);
void vc_depthcal_destroy(vc_depthcal* d);
/* size (w, h), bins, unit, kind, rect, v_ref, min_cos, max_dev, R_ck (row-major), t_ck; any pointer may be NULL */
int vc_depthcal_get(vc_depthcal* d, int size[2], int bins[2], double* unit, int* kind, double rect[4], double* v_ref, double* min_cos,
                    double* max_dev, double R_ck[9], double t_ck[3]);
/* sums, counters and the frame count back to zero; a fit that came from the sums is dropped */
int vc_depthcal_clear(vc_depthcal* d);
/* n depth images with their frames' poses T_wk (n x 7) added to the sums.  counters (nullable): n x 8, the table above, per frame.  One
 * upload, the launches and one synchronisation per call.  A pose that is not finite or not of unit length to 1e-6 is VC_ERR_BAD_ARG and
 * nothing is added.  A fit that came from the sums is dropped. */
int vc_depthcal_add(vc_depthcal* d, int n, const unsigned short* depth, int pitch, long long stride, const double* T_wk /* n x 7 */,
                    long long* counters /* n x 8, nullable */);
/* The per-pixel face, and the depth image the calibration predicts: y (n x h x w doubles) the expected value in counts, rule (n x h x w
 * bytes) the first rule that drops the pixel or 7; y = NaN under rules 1 and 2.  Without depth (NULL) rules 0 and 6 are not applied. */
int vc_depthcal_expected(vc_depthcal* d, int n, const double* T_wk /* n x 7 */, const unsigned short* depth /* nullable */, int pitch,
                         long long stride, double* y, unsigned char* rule);
/* sums: cells x 9; totals: the cells' sums added in cell order; the running counters; the frame count.  Any pointer may be NULL. */
int vc_depthcal_sums(vc_depthcal* d, double* sums, double totals[9], long long counters[8], long long* n_frames);
/* the fit of the sums as they stand (min_count >= 1, min_spread >= 0) */
int vc_depthcal_fit(vc_depthcal* d, int degree, int min_count, double min_spread);
/* c[3], a / b / status (cells each), rms[3], degree; any pointer may be NULL.  VC_ERR_BAD_ARG before a fit: adding frames or clearing
 * drops a fit that came from the sums, and nothing stale is returned. */
int vc_depthcal_get_fit(vc_depthcal* d, double c[3], double* a, double* b, int* status, double rms[3], int* degree);
/* a correction read from a file, for a fresh handle to apply: it stays until the next fit or set_fit (its rms are NaN) */
int vc_depthcal_set_fit(vc_depthcal* d, int degree, const double c[3], const double* a, const double* b);
/* n depth images corrected by the handle's fit (VC_ERR_BAD_ARG without one).  dst == src is allowed; a destination row's padding is not
 * written.  counters (nullable): n x 3 -- zeros in, values corrected, values out of range.  One upload, one launch, one download and one
 * synchronisation per call. */
int vc_depthcal_apply(vc_depthcal* d, int n, const unsigned short* src, int src_pitch, long long src_stride, unsigned short* dst, int dst_pitch,
                      long long dst_stride, int interp, long long* counters /* n x 3, nullable */);
/* HIP events on the handle's stream, `reps` launches each: out_ms[0] the table build, [1] accumulate + fold of n_images device-resident
 * images (into sums of the timer's own), [2] the apply. */
int vc_time_depthcal(vc_depthcal* d, int n_images, int reps, double out_ms[3]);

/* ---- the noise of an IMU from a log recorded at rest -----------------------------------------------------------------------------------
 * vc_set_sigmas takes two numbers that belong to the sensor, not to the calibration.  The overlapping Allan variance of a static log
 * gives them.  A handle holds one log of n samples (2 <= n <= 2^24; more is VC_ERR_UNSUPPORTED, before anything is read) on six channels
 * gx gy gz ax ay az: on the device, per channel, the mean and S_0 = 0, S_k = sum_{i<k} (y_i - mean).  For an averaging factor m over the
 * samples [first, first + count) in use
 *   avar(m) = sum_{k=first}^{first+count-2m} (S_{k+2m} - 2 S_{k+m} + S_k)^2 / (2 m^2 terms),   terms = count - 2m + 1,
 * at the averaging time tau = m tau0, tau0 = (t_{n-1} - t_0) / (n - 1).  Everything is fp64; no sum's order depends on anything but n, the
 * range and m: two runs give the same bits, and a channel's bits do not depend on the other five.
 * VC_ERR_BAD_ARG comes before any device call: a null pointer, n < 2, a time that is not finite or not strictly increasing, a sample
 * that is not finite.  VC_ERR_NO_DEVICE without a device: there is no host fallback.  A handle is single-threaded. */
typedef struct vc_allan vc_allan;
int vc_allan_create(int device, int n, const double* gyro /* n x 3 */, const double* accel /* n x 3 */, const double* time /* n */, vc_allan** out);
void vc_allan_destroy(vc_allan* a);
/* n, tau0, the smallest and largest interval, the six means, the number of intervals outside [0.5, 1.5] tau0 (reported, not refused), the
 * range in use (first, count); any pointer may be NULL */
int vc_allan_get(vc_allan* a, int* n, double* tau0, double* dt_min, double* dt_max, double means[6], long long* irregular, int range[2]);
/* The part of the log that is a static log.  Window start k (0 <= k <= n - 2 window) is quiet when the mean over `window` samples changes
 * by less than the threshold to the next window on both sensors: the norm over the sensor's three axes of
 * (S_{k+2W} - 2 S_{k+W} + S_k) / W.  The longest run of consecutive quiet starts k0 .. k1, the earliest among equals, becomes the range:
 * samples [k0, k1 + 2 window).  A threshold <= 0 switches that sensor's test off; both off: the whole log.  range_out (nullable): first,
 * count; n_quiet (nullable): quiet starts in the log.  Returns 1, the range unchanged, when no start is quiet.  VC_ERR_BAD_ARG:
 * window < 1, 2 window >= n, a threshold that is NaN. */
int vc_allan_static(vc_allan* a, int window, double gyro_thr, double accel_thr, int range_out[2], int* n_quiet);
/* VC_ERR_BAD_ARG: a range outside the log or shorter than 2 */
int vc_allan_set_range(vc_allan* a, int first, int count);
/* avar[c * n_m + j] of channel c at factor m[j] over the range in use; terms (nullable): n_m.  VC_ERR_BAD_ARG: n_m outside 1 .. 65535, a
 * factor with m < 1 or 2 m > count. */
int vc_allan_run(vc_allan* a, int n_m, const int* m, double* avar /* 6 x n_m */, int* terms /* n_m, nullable */);
/* HIP events on the handle's stream, `reps` launches back to back each: out_ms[0] the means and prefix sums, [1] the sweep of vc_allan_run
 * over the range in use.  The same input: the same bits are written again. */
int vc_time_allan(vc_allan* a, int n_m, const int* m, int reps, double out_ms[2]);
/* Host only, no device, no handle.  The averaging factors round(10^(j / per_decade)), j = 0, 1, ..., made strictly increasing, up to
 * max(1, floor(n_used max_fraction)); rel_err (nullable): IEEE Std 952's relative standard error of adev, 1 / sqrt(2 (n_used / m - 1)).
 * *n_m is the count; with m == NULL nothing else is written.  VC_ERR_BAD_ARG: n_used < 2, per_decade < 1, max_fraction outside
 * (0, 0.5], a count above cap. */
int vc_allan_factors(int n_used, int per_decade, double max_fraction, int cap, int* m, double* rel_err, int* n_m);
/* Host only.  avar(tau) = N^2 / tau + (2 ln 2 / pi) B^2 + K^2 tau / 3 fitted to n points with weights 1 / (avar^2 rel_err^2), N, B, K >= 0:
 * the seven non-empty subsets of the terms by their normal equations; of the non-negative solutions the smallest weighted residual.
 * out[5] = N (white noise, unit / sqrt(Hz)), B (bias instability), K (rate random walk), the rms of log(model / measured), the number of
 * points used (a point whose tau, avar or rel_err is not positive and finite is left out); mask: bit 0 N, bit 1 B, bit 2 K active.
 * Returns 0, 1 (fewer than three points, the model's terms: nothing fitted) or 2 (no feasible subset); VC_ERR_BAD_ARG: a null pointer, n < 1. */
int vc_allan_fit(int n, const double* tau, const double* avar, const double* rel_err, double out[5], int* mask);

/* ---- the inertial seed: camera-IMU rotation, time offset, gyro bias and gravity before anything is solved ------------------------------
 * On the device, no handle.  The frames bring the camera's rotation in the world (frame_q_wc, [x y z w], e.g. from vc_pnp_planar_batch;
 * frame_ok = 0: a frame without one), the log n_samples (2 .. 2^24; more is VC_ERR_UNSUPPORTED) of gyro and accelerometer.  A sample stamped
 * t was taken at image-clock time t + offset, T_wk = T_wc T_ck and w_c = R_ck (z_g + b_g): the scale factors are taken as 1.
 *   a_i    = log(R_wc,i^T R_wc,i+1) / (t_{i+1} - t_i), valid when both frames are ok and 0 < t_{i+1} - t_i <= max_gap_s
 *   b_i(d) = the mean of the piecewise-linear gyro signal over [t_i - d, t_{i+1} - d], from its prefix integrals; an interval that leaves
 *            the log is not valid at that lag
 * Per lag d, over the n valid intervals: R = Horn's rotation with a - am = R (b - bm), J = sum |R (b - bm) - (a - am)|^2 / n evaluated as
 * (Sa + Sb - 2 tr(R H)) / n, bias = R^T am - bm.  A lag with fewer than max(3, min_intervals) intervals has J = +inf, R = I, bias = 0; its
 * count is still returned.  moments (18 per lag): n, sum a', sum b, sum |a'|^2, sum |b|^2, sum b a'^T (row-major), a' = a minus the rate of
 * the first valid interval.  Any output pointer may be NULL.  Everything is fp64; no sum's order depends on anything but the sizes: two
 * runs give the same bits, a lag gives the same bits alone or among others, and the gyro channels permuted cyclically give the same J
 * bits with the columns of R permuted.
 * VC_ERR_BAD_ARG comes before any device call: a null required pointer, n_frames < 2, n_samples < 2, n_lags < 1, a time that is not finite
 * or not strictly increasing (frames and samples), a sample or a lag that is not finite, a quaternion of an ok frame with a norm outside
 * [0.5, 2], max_gap_s <= 0, min_intervals < 1.  VC_ERR_NO_DEVICE without that device: there is no host fallback. */
int vc_seed_imu_sweep(int device, int n_frames, const double* frame_t, const double* frame_q_wc /* n_frames x 4 */, const unsigned char* frame_ok,
                      int n_samples, const double* imu_t, const double* gyro /* n_samples x 3 */, const double* accel /* n_samples x 3 */,
                      double max_gap_s, int min_intervals, int n_lags, const double* lags,
                      double* J, double* R /* n_lags x 9 */, double* bias /* n_lags x 3 */, int* count, double* moments /* n_lags x 18 */);
/* The seed.  A coarse lattice of lags -range_s .. +range_s at step_s (<= 0: the median sample interval), the lowest J (the lowest index
 * among equals); a fine lattice of 4 fine + 1 lags at step_s / fine around it and a parabola through the three points around its minimum;
 * one more lag at the refined offset gives R_ck (row-major), gyro_bias, rms = sqrt(J), signal = sqrt(Sa / n), count.  Gravity at that
 * (R_ck, offset): u = normalise(sum R_wc,i R_ck abar_i), abar_i the mean accelerometer reading over the interval; g_dir = (asin(u_y),
 * asin(-u_x / cos g_dir[0])) as vc_get_gravity reports it.
 * status: 0 ok; 1 fewer than max(3, min_intervals) valid intervals at every lag; 2 the minimum lies on the edge of the range (the offset
 * is outside it); 3 a result that is not finite.  With a status other than 0 only status and the coarse curve are written.  rms / signal
 * near 1 means the rates do not explain each other: the caller declines the seed.  The coarse curve: coarse_cap entries of room in
 * coarse_lags / coarse_J (either may be NULL), *n_coarse (nullable) the lattice's size.  VC_ERR_BAD_ARG as vc_seed_imu_sweep, and for
 * range_s <= 0, fine < 1, a lattice of more than 2^20 lags, status == NULL. */
int vc_seed_imu(int device, int n_frames, const double* frame_t, const double* frame_q_wc, const unsigned char* frame_ok, int n_samples,
                const double* imu_t, const double* gyro, const double* accel, double max_gap_s, int min_intervals, double range_s, double step_s,
                int fine, double* time_offset, double R_ck[9], double gyro_bias[3], double g_dir[2], double* rms, double* signal, int* count,
                int* status, int coarse_cap, double* coarse_lags, double* coarse_J, int* n_coarse);
/* Mean kernel times in ms, `reps` launches back to back between two events each: out_ms[0] the prefix integrals and the camera rates,
 * [1] the sweep of those lags with its finishing kernel, [2] the gravity sums at lags[0]. */
int vc_time_seed_imu(int device, int n_frames, const double* frame_t, const double* frame_q_wc, const unsigned char* frame_ok, int n_samples,
                     const double* imu_t, const double* gyro, const double* accel, double max_gap_s, int min_intervals, int n_lags,
                     const double* lags, int reps, double out_ms[3]);

/* ---- the rig seed: every camera's pose relative to camera 0 from the views it shares, before anything is solved ------------------------
 * On the device, no handle.  The input is poses, wherever they come from: view_T_cw[k][c] = [qx qy qz qw tx ty tz] takes the target into
 * camera c at frame k (a unit quaternion, e.g. from vc_pnp_planar_batch), view_ok[k][c] = 0: no such view; its pose is never read into a
 * result (it may be NaN).  Pairs are (a < b) in the order (0,1), (0,2) .. (0,C-1), (1,2) ..; n_pairs = C (C - 1) / 2.  n_cams up to 8,
 * n_frames up to 131072; more is VC_ERR_UNSUPPORTED.
 * Per pair, every frame k with both views ok gives a candidate X_k = T_aw(k) T_bw(k)^-1 (camera b into camera a; the quaternion
 * normalised) with the scale d_k = max(|t_aw(k)|, |t_bw(k)|).  Candidates i and j agree when |q_i . q_j| >= cos(tol / 2) and
 * |t_i - t_j|^2 <= tol_rad^2 (d_i + d_j)^2: one angular tolerance serves both, since a pose error of angle e moves the camera by about e
 * times its distance to the target.  The support of i is the number of shared frames that agree with it, itself included; the winner has
 * the largest support, the lowest frame among equals.  The refit over the winner's agreeing frames: q = normalise(sum s_j q_j), s_j = -1
 * where q_j . q_winner < 0, with qw >= 0; t the mean of t_j; pair_rms_deg the rms of the angles 2 atan2(|vec|, |w|) of q^-1 q_j,
 * pair_rms_m the rms of |t_j - t|.  pair_shared: the frames both cameras see; pair_winner: the winner's frame.
 * pair_status: 0 ok, 1 no shared frame, 2 support below min_support; with a status other than 0 only pair_shared and pair_status are
 * written.
 * The rig (host code): a maximum spanning tree over the status-0 pairs weighted by support, grown from camera 0 by Prim's rule, ties to
 * the lowest tree camera, then the lowest new camera.  cam_T_c0[c] takes camera 0 into camera c, composed along the tree (qw >= 0;
 * camera 0: the identity); cam_parent: -1 for camera 0 and for a camera not reached; cam_status: 0 reached, 1 not connected (its pose is
 * left as it was).
 * Everything is fp64, the supports are integers, no sum's order depends on anything but the pair's own shared frames: two runs give the
 * same bits, and a pair gives the same bits whatever other cameras are in the batch.
 * VC_ERR_BAD_ARG comes before any device call: a null pointer, n_frames < 0, n_cams < 1, tol_deg outside (0, 90), min_support < 1.
 * VC_ERR_NO_DEVICE without that device: there is no host fallback. */
int vc_seed_rig(int device, int n_frames, int n_cams, const unsigned char* view_ok /* n_frames x n_cams */,
                const double* view_T_cw /* n_frames x n_cams x 7 */, double tol_deg, int min_support,
                double* pair_T_ab /* n_pairs x 7 */, int* pair_shared, int* pair_support, int* pair_winner, double* pair_rms_deg, double* pair_rms_m,
                int* pair_status, double* cam_T_c0 /* n_cams x 7 */, int* cam_parent, int* cam_status);
/* Mean kernel times in ms, `reps` launches back to back between two events each: kernel_ms[0] the candidates, [1] the vote (quadratic in
 * the shared frames), [2] the winner and the refit.  All zero when no pair shares a frame.  VC_ERR_BAD_ARG also for reps < 1. */
int vc_time_seed_rig(int device, int n_frames, int n_cams, const unsigned char* view_ok, const double* view_T_cw, double tol_deg, int min_support,
                     int reps, double kernel_ms[3]);

#ifdef __cplusplus
}
#endif
#endif /* VICALIB_AMD_H_ */
