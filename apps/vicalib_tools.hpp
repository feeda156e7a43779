// The command-line tool's file-to-file tools and the writers that run behind a calibration, each with the check of its flags.  A piece of
// vicalib.cpp's translation unit: that file includes it behind vicalib_flags.hpp and vicalib_io.hpp, nothing else does.
#pragma once
// -undistort_dir: every input image of every camera through the calibrated model into a pinhole camera of the same size (intrinsics from
// vc_undistort_fit_linear at -undistort_alpha), in batches of at most 64 images per call; dir/cameras.xml is the rig with every camera
// replaced by that pinhole camera, T_ck kept, written by the calibrator's own XML writer
static bool UndistortInputs(vic::ViCalibrator& cal, const std::vector<std::string>& cam_globs, const std::vector<vic::CameraAndPose>& input_cameras,
                            bool calibrate_imu, int device, const std::string& dir, double alpha, std::string* err) {
  if (!MakeDir(dir, err)) return false;               // (one level: parents must exist)
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
      for (size_t k = 0; k < n; ++k)
        if (!WritePgm(dir + "/cam" + std::to_string(c) + "_" + BaseName(files[first + k]) + ".pgm", w, h, out.data() + k * np, err)) return false;
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

// -rectify_dir: cameras a and b of the result rectified (vc_rectifier: the rotations of vc_stereo_rectify_rotations, one pinhole camera of
// a's size for both from vc_stereo_fit_linear at -rectify_alpha).  dir/cameras.xml holds the two rectified cameras (T_ck_rect: they differ by
// a translation along x), dir/stereo_check.csv the stereo consistency check over the corners both cameras detected in the frames the
// calibration used, and with image input the i-th sorted image of a and of b are rectified as a pair, in batches of at most 64.
static bool RectifyOutputs(vic::ViCalibrator& cal, const std::vector<Channel>& channels, const std::vector<long>& frame_ids, int grid_n,
                           const std::vector<std::string>& cam_globs, bool from_images, const std::vector<vic::CameraAndPose>& input_cameras, bool calibrate_imu,
                           int device, const std::string& dir, int a, int b, double alpha, std::string* err) {
  if (!MakeDir(dir, err)) return false;                  // (one level: parents must exist)
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
  std::vector<int> tile_frame, tile_cam, point_id;
  std::vector<long long> tile_off(1, 0);
  std::vector<const Detection*> dets;
  for (int s = 0; s < 2; ++s) {
    for (const auto& kv : DetectionsByFrame(channels[(size_t)cams[s]], FrameIndex(frame_ids), grid_n)) {
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
  if (!ComparableRigs(A, B, o, err) || !MakeDir(o.dir, err)) return 1;
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
  if (!MakeDir(o.dir, err)) return 1;
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
  if (!MakeDir(o.dir, err)) return false;
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
  if (!MakeDir(o.dir, err)) return false;
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
  if (!MakeDir(o.dir, err)) return false;
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
