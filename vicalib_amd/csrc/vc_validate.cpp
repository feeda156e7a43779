// vc_validate.cpp -- held-out scoring behind vc_holdout_* (include/vicalib_amd.h).  The hold-out set lives beside the problem, not in
// it: its own host vectors (vc_calibrator::Holdout), its own device buffers, allocated at the first compute.  It reads the cameras from
// the host state (what vc_get_camera returns), never uploads or invalidates the solve's problem, never touches the trace, the
// iteration counters or the residual report, and launches its two kernels (vc_validate.hip) on the calibrator's stream.
#include "vc_calibrator.hpp"

// Seeds of the frames from their own detections, as vc_init_frame_poses_pnp seeds the frames of the problem: camera 0 if it has >= 4
// corners, otherwise the last camera that has; T_wk = T_cw^-1 * T_ck.  ok[f] = 0 where no view gave a pose.
static void holdout_pnp_seeds(const vc_calibrator* h, const vc_calibrator::Holdout& ho, const std::vector<int>& order, const std::vector<int>& tile_frame,
                              const std::vector<int>& tile_cam, const std::vector<int>& tile_off, std::vector<double>* seeds, std::vector<int>* ok) {
  std::vector<double> pw, pc;
  std::vector<char> cam0_good((size_t)ho.n_frames, 0);
  for (size_t t = 0; t < tile_frame.size(); ++t) {             // tiles are ordered by frame, then camera
    const int f = tile_frame[t], c = tile_cam[t], n = tile_off[t + 1] - tile_off[t];
    if (n < 4) continue;
    if (c != 0 && cam0_good[f]) continue;
    pw.resize(3 * (size_t)n); pc.resize(2 * (size_t)n);
    for (int k = 0; k < n; ++k) {
      const size_t i = (size_t)order[tile_off[t] + k];
      std::memcpy(&pw[3 * (size_t)k], &ho.pts.xyz[3 * (size_t)ho.o_pid[i]], 24); std::memcpy(&pc[2 * (size_t)k], &ho.o_pc[2 * i], 16);
    }
    const HostCam& cm = h->cams[c];
    double T_cw[7], rms;
    if (!pnp_planar_ransac(cm.model, cm.K, n, pw.data(), pc.data(), h->pnp_its, h->pnp_tol, T_cw, &rms, nullptr, nullptr)) continue;
    const double qi[4] = {-T_cw[0], -T_cw[1], -T_cw[2], T_cw[3]};
    const double nt[3] = {-T_cw[4], -T_cw[5], -T_cw[6]};
    double ti[3], tr[3];
    double* T = seeds->data() + (size_t)f * kPoseStride;
    quat_rotate(qi, nt, ti);
    quat_mul(qi, cm.T_ck, T);
    quat_rotate(qi, cm.T_ck + 4, tr);
    for (int k = 0; k < 3; ++k) T[4 + k] = ti[k] + tr[k];
    (*ok)[f] = 1;
    if (c == 0) cam0_good[f] = 1;
  }
}

// The same seeds with the switch of vc_set_pnp_device on: every tile of >= 4 corners in one batch on the calibrator's device, the rule above
// applied to the statuses on the host.
static int holdout_pnp_seeds_device(vc_calibrator* h, const vc_calibrator::Holdout& ho, const std::vector<int>& order, const std::vector<int>& tile_frame,
                                    const std::vector<int>& tile_cam, const std::vector<int>& tile_off, std::vector<double>* seeds, std::vector<int>* ok) {
  std::vector<int> v_tile, v_cam, v_off(1, 0);
  std::vector<double> pw, pc;
  for (size_t t = 0; t < tile_frame.size(); ++t) {
    const int n = tile_off[t + 1] - tile_off[t];
    if (n < 4) continue;
    for (int k = 0; k < n; ++k) {
      const size_t i = (size_t)order[tile_off[t] + k];
      pw.insert(pw.end(), &ho.pts.xyz[3 * (size_t)ho.o_pid[i]], &ho.pts.xyz[3 * (size_t)ho.o_pid[i]] + 3);
      pc.insert(pc.end(), &ho.o_pc[2 * i], &ho.o_pc[2 * i] + 2);
    }
    v_tile.push_back((int)t); v_cam.push_back(tile_cam[t]); v_off.push_back((int)(pc.size() / 2));
  }
  std::vector<double> T_all;
  std::vector<int> status;
  const int rc = h->pnp_batch(v_cam, v_off, pw, pc, &T_all, &status);
  if (rc != VC_OK) return rc;
  std::vector<char> cam0_good((size_t)std::max(ho.n_frames, 1), 0);
  for (size_t v = 0; v < v_tile.size(); ++v) {                  // (ordered by frame, then camera)
    const int f = tile_frame[v_tile[v]], c = v_cam[v];
    if ((c != 0 && cam0_good[f]) || status[v] != 0) continue;
    const HostCam& cm = h->cams[c];
    const double* T_cw = &T_all[7 * v];
    const double qi[4] = {-T_cw[0], -T_cw[1], -T_cw[2], T_cw[3]};
    const double nt[3] = {-T_cw[4], -T_cw[5], -T_cw[6]};
    double ti[3], tr[3];
    double* T = seeds->data() + (size_t)f * kPoseStride;
    quat_rotate(qi, nt, ti);
    quat_mul(qi, cm.T_ck, T);
    quat_rotate(qi, cm.T_ck + 4, tr);
    for (int k = 0; k < 3; ++k) T[4 + k] = ti[k] + tr[k];
    (*ok)[f] = 1;
    if (c == 0) cam0_good[f] = 1;
  }
  return VC_OK;
}

int vc_calibrator::holdout_compute(const double* seeds_in, int iters) {
  HIP_OK(hipSetDevice(device));
  Holdout& ho = hold;
  ho.valid = false;
  const int F = ho.n_frames, C = (int)cams.size();
  const size_t n = ho.o_frame.size();
  if (C < 1 || C > kMaxCams) return VC_ERR_BAD_ARG;
  // ---- tiles: the corners grouped by (frame, camera), in order of arrival inside a group ---------------------------------
  std::vector<int> order(n);
  for (size_t i = 0; i < n; ++i) order[i] = (int)i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    return ho.o_frame[a] != ho.o_frame[b] ? ho.o_frame[a] < ho.o_frame[b] : ho.o_cam[a] < ho.o_cam[b];
  });
  std::vector<int> tile_frame, tile_cam, tile_off, frame_tile_off((size_t)F + 1, 0), pt(n);
  std::vector<double2> uv(n);
  for (size_t k = 0; k < n; ++k) {
    const int i = order[k];
    if (k == 0 || ho.o_frame[i] != ho.o_frame[order[k - 1]] || ho.o_cam[i] != ho.o_cam[order[k - 1]]) {
      tile_frame.push_back(ho.o_frame[i]); tile_cam.push_back(ho.o_cam[i]); tile_off.push_back((int)k);
      frame_tile_off[(size_t)ho.o_frame[i] + 1] += 1;
    }
    uv[k] = make_double2(ho.o_pc[2 * (size_t)i], ho.o_pc[2 * (size_t)i + 1]); pt[k] = ho.o_pid[i];
  }
  tile_off.push_back((int)n);
  for (int f = 0; f < F; ++f) frame_tile_off[(size_t)f + 1] += frame_tile_off[f];
  const int T = (int)tile_frame.size();
  // ---- seeds -----------------------------------------------------------------------------------------------------
  std::vector<double> seeds((size_t)std::max(F, 1) * kPoseStride, 0.0);
  std::vector<int> seed_ok(std::max(F, 1), 0);
  for (int f = 0; f < F; ++f) seeds[(size_t)f * kPoseStride + 3] = 1.0;
  if (seeds_in) {
    for (int f = 0; f < F; ++f) { std::memcpy(&seeds[(size_t)f * kPoseStride], seeds_in + 7 * (size_t)f, 56); seed_ok[f] = 1; }
  } else if (pnp_device) {
    const int rc = holdout_pnp_seeds_device(this, ho, order, tile_frame, tile_cam, tile_off, &seeds, &seed_ok);
    if (rc != VC_OK) return rc;
  } else {
    holdout_pnp_seeds(this, ho, order, tile_frame, tile_cam, tile_off, &seeds, &seed_ok);
  }
  // ---- the frozen cameras, from the host state ---------------------------------------------------------------------
  std::vector<double> cam_rec((size_t)C * kCamStride, 0.0);
  HoldoutView v{};
  for (int c = 0; c < kMaxCams; ++c) v.model[c] = kLinear;
  for (int c = 0; c < C; ++c) {
    std::memcpy(&cam_rec[(size_t)c * kCamStride], cams[c].T_ck, 56);
    std::memcpy(&cam_rec[(size_t)c * kCamStride + kCamK], cams[c].K, (size_t)cams[c].nk * 8);
    v.model[c] = cams[c].model;
  }
  v.n_frames = F; v.n_tiles = T; v.n_cams = C;
  v.max_iters = iters <= 0 ? kHoldoutDefaultIters : std::min(iters, kHoldoutMaxIters);
  v.ftol = function_tolerance; v.gtol = gradient_tolerance; v.ptol = parameter_tolerance;
  HIP_OK(ho.d_cams.upload(cam_rec, stream)); HIP_OK(ho.d_points.upload(ho.pts.xyz, stream));
  HIP_OK(ho.d_frame_tile_off.upload(frame_tile_off, stream)); HIP_OK(ho.d_tile_frame.upload(tile_frame, stream));
  HIP_OK(ho.d_tile_cam.upload(tile_cam, stream)); HIP_OK(ho.d_tile_off.upload(tile_off, stream));
  HIP_OK(ho.d_uv.upload(uv, stream)); HIP_OK(ho.d_pt.upload(pt, stream)); HIP_OK(ho.d_obs_index.upload(order, stream));
  HIP_OK(ho.d_seeds.upload(seeds, stream)); HIP_OK(ho.d_seed_ok.upload(seed_ok, stream));
  HIP_OK(ho.d_pose.alloc((size_t)std::max(F, 1) * kPoseStride)); HIP_OK(ho.d_frame_int.alloc((size_t)std::max(F, 1) * 3));
  HIP_OK(ho.d_cost.alloc((size_t)std::max(F, 1) * 2)); HIP_OK(ho.d_res.alloc(std::max<size_t>(n, 1)));
  HIP_OK(ho.d_view.alloc((size_t)std::max(T, 1) * 2)); HIP_OK(ho.d_worst.alloc(std::max(T, 1)));
  v.cams = ho.d_cams.p; v.points = ho.d_points.p; v.frame_tile_off = ho.d_frame_tile_off.p; v.tile_frame = ho.d_tile_frame.p;
  v.tile_cam = ho.d_tile_cam.p; v.tile_off = ho.d_tile_off.p; v.obs_uv = ho.d_uv.p; v.obs_pt = ho.d_pt.p; v.obs_index = ho.d_obs_index.p;
  v.seeds = ho.d_seeds.p; v.seed_ok = ho.d_seed_ok.p;
  v.pose = ho.d_pose.p; v.status = ho.d_frame_int.p; v.iters = ho.d_frame_int.p + std::max(F, 1); v.behind = ho.d_frame_int.p + 2 * (size_t)std::max(F, 1);
  v.cost = ho.d_cost.p; v.res = ho.d_res.p; v.view_sq = ho.d_view.p; v.view_max = ho.d_view.p + std::max(T, 1); v.view_worst = ho.d_worst.p;
  launch_validate_pose(v, stream);
  launch_validate_residuals(v, stream);
  HIP_OK(hipGetLastError());
  // ---- the small results to the host; the corners stay on the device (vc_holdout_corners reads slices) -------------------------
  std::vector<double> pose((size_t)std::max(F, 1) * kPoseStride), cost((size_t)std::max(F, 1) * 2), view((size_t)std::max(T, 1) * 2);
  std::vector<int> fint((size_t)std::max(F, 1) * 3);
  ho.v_worst.assign(T, -1);
  if (F) {
    HIP_OK(hipMemcpyAsync(pose.data(), ho.d_pose.p, pose.size() * 8, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(cost.data(), ho.d_cost.p, cost.size() * 8, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(fint.data(), ho.d_frame_int.p, fint.size() * 4, hipMemcpyDeviceToHost, stream));
  }
  if (T) {
    HIP_OK(hipMemcpyAsync(view.data(), ho.d_view.p, view.size() * 8, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(ho.v_worst.data(), ho.d_worst.p, (size_t)T * 8, hipMemcpyDeviceToHost, stream));
  }
  HIP_OK(hipStreamSynchronize(stream));
  ho.f_pose.resize((size_t)F * 7); ho.f_status.resize(F); ho.f_iters.resize(F); ho.f_behind.resize(F); ho.f_cost0.resize(F); ho.f_cost.resize(F);
  for (int f = 0; f < F; ++f) {
    std::memcpy(&ho.f_pose[(size_t)f * 7], &pose[(size_t)f * kPoseStride], 56);
    ho.f_status[f] = fint[f]; ho.f_iters[f] = fint[(size_t)F + f]; ho.f_behind[f] = fint[2 * (size_t)F + f];
    ho.f_cost0[f] = cost[f]; ho.f_cost[f] = cost[(size_t)F + f];
  }
  ho.v_frame = tile_frame; ho.v_cam = tile_cam; ho.v_count.resize(T); ho.v_sq.resize(T); ho.v_max.resize(T);
  for (int t = 0; t < T; ++t) { ho.v_count[t] = tile_off[t + 1] - tile_off[t]; ho.v_sq[t] = view[t]; ho.v_max[t] = view[(size_t)std::max(T, 1) + t]; }
  ho.cams_used = cams;
  ho.last = v;
  ho.valid = true;
  return VC_OK;
}

#define NOT_RUNNING(h) do { if (!(h)) return VC_ERR_BAD_ARG; if ((h)->is_running) return VC_ERR_RUNNING; } while (0)
// the scores can be read while they describe the hold-out set and the cameras: computed, and neither changed since (a camera the host
// state no longer holds bit for bit -- a solve, vc_download_state -- is a change)
static bool holdout_current(const vc_calibrator* h) {
  const vc_calibrator::Holdout& ho = h->hold;
  if (!ho.valid || ho.cams_used.size() != h->cams.size()) return false;
  for (size_t c = 0; c < h->cams.size(); ++c) if (std::memcmp(&ho.cams_used[c], &h->cams[c], sizeof(HostCam)) != 0) return false;
  return true;
}
#define HOLDOUT_READY(h) do { NOT_RUNNING(h); if (!holdout_current(h)) return VC_ERR_BAD_ARG; } while (0)

extern "C" {

int vc_holdout_clear(vc_calibrator* h) {
  NOT_RUNNING(h);
  if (hipSetDevice(h->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  h->hold.release();
  return VC_OK;
}
int vc_holdout_add_tiles(vc_calibrator* h, int n_tiles, const int* tile_frame, const int* tile_cam, const long long* tile_off, const double* points,
                         int n_points, const int* point_id, const double* p_c) {
  NOT_RUNNING(h);
  if (n_tiles < 0 || (n_tiles > 0 && (!tile_frame || !tile_cam || !tile_off)) || n_points < 0) return VC_ERR_BAD_ARG;
  if (n_tiles == 0) return VC_OK;
  const int C = (int)h->cams.size();
  if (tile_off[0] < 0) return VC_ERR_BAD_ARG;
  for (int t = 0; t < n_tiles; ++t)
    if (tile_frame[t] < 0 || tile_frame[t] >= (1 << 24) || tile_cam[t] < 0 || tile_cam[t] >= C || tile_off[t + 1] < tile_off[t]) return VC_ERR_BAD_ARG;
  const long long n0 = tile_off[0], n1 = tile_off[n_tiles];
  if (n1 > n0 && (!points || !point_id || !p_c)) return VC_ERR_BAD_ARG;
  vc_calibrator::Holdout& ho = h->hold;
  if ((long long)ho.o_frame.size() + (n1 - n0) > 0x7fffffffLL) return VC_ERR_UNSUPPORTED;
  for (long long i = n0; i < n1; ++i) if (point_id[i] < 0 || point_id[i] >= n_points) return VC_ERR_BAD_ARG;
  // the points this call's corners use join the set's table; more than the problem itself may hold is refused with the set unchanged
  const size_t old_pts = (size_t)ho.pts.size();
  std::vector<int> remap((size_t)n_points, -1);
  for (long long i = n0; i < n1; ++i) if (remap[point_id[i]] < 0) remap[point_id[i]] = ho.pts.intern(points + 3 * (size_t)point_id[i]);
  if (ho.pts.size() > kObsPointMask + 1) {
    PointTable before;
    for (size_t i = 0; i < old_pts; ++i) before.intern(&ho.pts.xyz[3 * i]);
    ho.pts = before;
    return VC_ERR_TOO_MANY_POINTS;
  }
  ho.valid = false;
  const size_t add = (size_t)(n1 - n0), base = ho.o_frame.size();
  ho.o_frame.resize(base + add); ho.o_cam.resize(base + add); ho.o_pid.resize(base + add);
  for (int t = 0; t < n_tiles; ++t) {
    ho.n_frames = std::max(ho.n_frames, tile_frame[t] + 1);                 // (a tile of no corners still names a frame)
    for (long long i = tile_off[t]; i < tile_off[t + 1]; ++i) {
      const size_t k = base + (size_t)(i - n0);
      ho.o_frame[k] = tile_frame[t]; ho.o_cam[k] = tile_cam[t]; ho.o_pid[k] = remap[point_id[i]];
    }
  }
  if (add) ho.o_pc.insert(ho.o_pc.end(), p_c + 2 * n0, p_c + 2 * n1);
  return VC_OK;
}
int vc_holdout_compute(vc_calibrator* h, const double* seeds, int max_iters) {
  NOT_RUNNING(h);
  return h->holdout_compute(seeds, max_iters);
}
int vc_holdout_num_frames(vc_calibrator* h) { HOLDOUT_READY(h); return (int)h->hold.f_status.size(); }
int vc_holdout_num_views(vc_calibrator* h) { HOLDOUT_READY(h); return (int)h->hold.v_frame.size(); }
long long vc_holdout_num_corners(vc_calibrator* h) { HOLDOUT_READY(h); return (long long)h->hold.o_frame.size(); }
int vc_holdout_frames(vc_calibrator* h, double* T_wk, int* status, int* iterations, double* cost0, double* cost, int* behind) {
  HOLDOUT_READY(h);
  const vc_calibrator::Holdout& ho = h->hold;
  const size_t F = ho.f_status.size();
  if (T_wk) std::memcpy(T_wk, ho.f_pose.data(), F * 56);
  if (status) std::memcpy(status, ho.f_status.data(), F * sizeof(int));
  if (iterations) std::memcpy(iterations, ho.f_iters.data(), F * sizeof(int));
  if (cost0) std::memcpy(cost0, ho.f_cost0.data(), F * sizeof(double));
  if (cost) std::memcpy(cost, ho.f_cost.data(), F * sizeof(double));
  if (behind) std::memcpy(behind, ho.f_behind.data(), F * sizeof(int));
  return VC_OK;
}
int vc_holdout_views(vc_calibrator* h, int* frame, int* camera, int* count, double* sum_sq, double* max_err, long long* worst_corner) {
  HOLDOUT_READY(h);
  const vc_calibrator::Holdout& ho = h->hold;
  const size_t V = ho.v_frame.size();
  if (frame) std::memcpy(frame, ho.v_frame.data(), V * sizeof(int));
  if (camera) std::memcpy(camera, ho.v_cam.data(), V * sizeof(int));
  if (count) std::memcpy(count, ho.v_count.data(), V * sizeof(int));
  if (sum_sq) std::memcpy(sum_sq, ho.v_sq.data(), V * sizeof(double));
  if (max_err) std::memcpy(max_err, ho.v_max.data(), V * sizeof(double));
  if (worst_corner) std::memcpy(worst_corner, ho.v_worst.data(), V * sizeof(long long));
  return VC_OK;
}
int vc_holdout_corners(vc_calibrator* h, long long first, long long n, double* r, int* frame, int* camera) {
  HOLDOUT_READY(h);
  vc_calibrator::Holdout& ho = h->hold;
  if (first < 0 || n < 0 || first + n > (long long)ho.o_frame.size()) return VC_ERR_BAD_ARG;
  for (long long i = 0; i < n; ++i) {
    if (frame) frame[i] = ho.o_frame[(size_t)(first + i)];
    if (camera) camera[i] = ho.o_cam[(size_t)(first + i)];
  }
  if (!r || n == 0) return VC_OK;
  if (hipSetDevice(h->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  if (!ho.stage && hipHostMalloc((void**)&ho.stage, vc_calibrator::Holdout::kStageCorners * sizeof(double2), hipHostMallocDefault) != hipSuccess) return VC_ERR_NO_DEVICE;
  for (long long done = 0; done < n;) {
    const size_t m = (size_t)std::min<long long>(n - done, (long long)vc_calibrator::Holdout::kStageCorners);
    if (hipMemcpyAsync(ho.stage, ho.d_res.p + first + done, m * sizeof(double2), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
    std::memcpy(r + 2 * done, ho.stage, m * sizeof(double2));
    done += (long long)m;
  }
  return VC_OK;
}
int vc_holdout_camera_rmse(vc_calibrator* h, double* rmse, long long* count) {
  HOLDOUT_READY(h);
  const vc_calibrator::Holdout& ho = h->hold;
  const size_t C = h->cams.size();
  std::vector<double> sq(C, 0.0);
  std::vector<long long> cnt(C, 0);
  for (size_t t = 0; t < ho.v_frame.size(); ++t) {
    const int st = ho.f_status[ho.v_frame[t]];
    if (st != kHoConverged && st != kHoMaxIters) continue;      // views of flagged frames keep their rows and enter no camera sum
    sq[ho.v_cam[t]] += ho.v_sq[t]; cnt[ho.v_cam[t]] += ho.v_count[t];
  }
  for (size_t c = 0; c < C; ++c) {
    if (rmse) rmse[c] = cnt[c] > 0 ? std::sqrt(sq[c] / (2.0 * (double)cnt[c])) : 0.0;
    if (count) count[c] = cnt[c];
  }
  return VC_OK;
}
// Times the two kernels of the last vc_holdout_compute with HIP events on the calibrator's stream, `reps` launches each back to back
// (every launch starts from the seeds again: the results are rewritten with the same values)
int vc_time_holdout(vc_calibrator* h, int reps, double* out_ms) {
  HOLDOUT_READY(h);
  if (!out_ms || reps < 1) return VC_ERR_BAD_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  EventSet<3> evs;
  if (!evs.create()) return VC_ERR_NO_DEVICE;
  const HoldoutView& v = h->hold.last;
  hipStream_t s = h->stream;
  for (int w = 0; w < 2; ++w) {      // first round warms clocks and caches
    (void)hipEventRecord(evs.e[0], s); for (int i = 0; i < reps; ++i) launch_validate_pose(v, s);
    (void)hipEventRecord(evs.e[1], s); for (int i = 0; i < reps; ++i) launch_validate_residuals(v, s);
    (void)hipEventRecord(evs.e[2], s);
    if (hipEventSynchronize(evs.e[2]) != hipSuccess) return VC_ERR_NO_DEVICE;
  }
  for (int i = 0; i < 2; ++i) { float ms = 0; (void)hipEventElapsedTime(&ms, evs.e[i], evs.e[i + 1]); out_ms[i] = ms / reps; }
  return VC_OK;
}

}  // extern "C"
