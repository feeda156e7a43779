// vc_report.cpp -- the residual report behind vc_report_* (include/vicalib_amd.h): runs the report sweeps (vc_report.hip) at the accepted
// state, keeps the small results (view rows, error maps, IMU rows) on the host and the per-corner residuals on the device, from where
// vc_report_corners reads slices through a bounded page-locked buffer.  Nothing of the LM pass is touched: the sweeps read the state
// buffers and the observation arrays, and every buffer they write is the report's own.
#include "vc_calibrator.hpp"
#include <map>

void vc_calibrator::report_launch_imu(const ReportView& r) {
  Ctrl c;
  std::memset(&c, 0, sizeof(Ctrl));
  c.cur = r.cur; c.need_lin = 1;
  launch_set_ctrl(rep.d_ctrl.p, c, stream);
  DevView bv = dv;
  bv.ctrl = rep.d_ctrl.p; bv.imu_delta_blk = rep.d_delta.p; bv.imu_grav = rep.d_grav.p;
  bv.sync_seq = 0; bv.block_wait = 0; bv.final_wait = 0;
  launch_imu_delta(bv, stream, 0);
  launch_report_imu(dv, r, stream);
}

int vc_calibrator::report_compute(int bins_x, int bins_y) {
  HIP_OK(hipSetDevice(device));
  // upload() alone, not vc_prepare: a report before the first solve must not set the residual multiplicities that solve() counts up
  if (device_dirty) { int rc = upload(); if (rc) return rc; }
  rep.valid = false;
  const int T = dv.n_tiles, C = dv.n_cams, cells = bins_x * bins_y;
  const size_t n_all = o_frame.size(), n_obs = h_obs_index.size();
  // ---- the corners the outlier stage dropped: no longer on the device (vc_upload.cpp), evaluated by a side launch ---------------
  std::vector<ReportDropped> dropped;
  std::vector<double2> dropped_uv;
  for (size_t i = 0; i < n_all; ++i)
    if (o_removed[i] == 1) {
      dropped.push_back({o_frame[i], o_cam[i], o_pid[i], (int)i});
      dropped_uv.push_back(make_double2(o_pc[2 * i], o_pc[2 * i + 1]));
    }
  ReportView r{};
  r.cur = cur; r.wcur = wcur;
  HIP_OK(rep.d_res.alloc(std::max<size_t>(n_all, 1)));
  HIP_OK(rep.d_obs_index.upload(h_obs_index, stream));
  HIP_OK(rep.d_view.alloc((size_t)std::max(T, 1) * 2)); HIP_OK(rep.d_worst.alloc(std::max(T, 1))); HIP_OK(rep.d_marked.alloc(std::max(T, 1)));
  HIP_OK(rep.d_dropped.upload(dropped, stream)); HIP_OK(rep.d_dropped_uv.upload(dropped_uv, stream));
  r.res = rep.d_res.p; r.obs_index = rep.d_obs_index.p;
  r.view_sq = rep.d_view.p; r.view_max = rep.d_view.p + std::max(T, 1); r.view_worst = rep.d_worst.p; r.view_marked = rep.d_marked.p;
  r.n_dropped = (int)dropped.size(); r.dropped = rep.d_dropped.p; r.dropped_uv = rep.d_dropped_uv.p;
  r.bins_x = bins_x; r.bins_y = bins_y;
  // partial maps: as many as keep the first pass's grid wide (one wavefront per chunk and camera), within 64 MB of partial sums
  const int max_chunks = (int)std::max<size_t>(1, std::min<size_t>(kReportMapChunks, ((size_t)64 << 20) / ((size_t)std::max(C, 1) * cells * 4 * sizeof(double))));
  r.tiles_per_chunk = std::max(1, (T + max_chunks - 1) / max_chunks);
  r.n_chunks = std::max(1, (T + r.tiles_per_chunk - 1) / r.tiles_per_chunk);
  for (int c = 0; c < kMaxCams; ++c) { r.width[c] = c < C ? std::max(cams[c].width, 1) : 1; r.height[c] = c < C ? std::max(cams[c].height, 1) : 1; }
  HIP_OK(rep.d_map_part.alloc((size_t)r.n_chunks * std::max(C, 1) * cells * 4)); HIP_OK(rep.d_map.alloc((size_t)std::max(C, 1) * cells * 4));
  r.map_part = rep.d_map_part.p; r.map = rep.d_map.p;
  launch_report_vision(dv, r, stream);
  launch_report_map(dv, r, stream);
  // ---- IMU blocks: k_imu_block itself forms the delta records of the accepted state, on the report's buffers (a view of the problem
  // whose control record, delta records and gravity record are the report's; no flag hand-over) --------------------------------
  const int nb = dv.imu_on ? std::max(0, std::min(dv.n_frames - 1, vc_num_imu_blocks(this))) : 0;
  r.n_blocks = nb;
  if (nb > 0) {
    HIP_OK(rep.d_delta.alloc((size_t)std::max(dv.n_frames - 1, 1) * kBlockDeltaStride));      // (k_imu_block writes every block of the upload)
    HIP_OK(rep.d_grav.alloc(32)); HIP_OK(rep.d_ctrl.alloc(2));
    HIP_OK(rep.d_imu.alloc((size_t)nb * kReportImuCols)); HIP_OK(rep.d_imu_flags.alloc(nb));
    r.delta_blk = rep.d_delta.p; r.grav = rep.d_grav.p; r.imu_out = rep.d_imu.p; r.imu_flags = rep.d_imu_flags.p;
    report_launch_imu(r);
  }
  HIP_OK(hipGetLastError());
  // ---- the small results to the host -----------------------------------------------------------------------------------
  std::vector<double> view((size_t)std::max(T, 1) * 2);
  std::vector<long long> worst(std::max(T, 1));
  std::vector<int> marked(std::max(T, 1));
  rep.map.assign((size_t)C * cells * 4, 0.0); rep.imu.assign((size_t)nb * kReportImuCols, 0.0); rep.imu_flags.assign(nb, 0);
  if (T) {
    HIP_OK(hipMemcpyAsync(view.data(), rep.d_view.p, view.size() * 8, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(worst.data(), rep.d_worst.p, (size_t)T * 8, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(marked.data(), rep.d_marked.p, (size_t)T * 4, hipMemcpyDeviceToHost, stream));
  }
  if (C) HIP_OK(hipMemcpyAsync(rep.map.data(), rep.d_map.p, rep.map.size() * 8, hipMemcpyDeviceToHost, stream));
  if (nb) {
    HIP_OK(hipMemcpyAsync(rep.imu.data(), rep.d_imu.p, rep.imu.size() * 8, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(rep.imu_flags.data(), rep.d_imu_flags.p, (size_t)nb * 4, hipMemcpyDeviceToHost, stream));
  }
  HIP_OK(hipStreamSynchronize(stream));        // (also: the staging vectors above go out of scope)
  // ---- view rows: the tiles, plus the views whose every corner was dropped (no tile left), by frame, then camera ------------------
  std::map<long long, int> n_dropped_of;
  for (const ReportDropped& d : dropped) ++n_dropped_of[(long long)d.frame * kMaxCams + d.cam];
  struct Row { int frame, cam, count, removed; double sq, mx; long long worst; };
  std::vector<Row> rows;
  rows.reserve((size_t)T + n_dropped_of.size());
  for (int t = 0; t < T; ++t) {
    const long long key = (long long)h_tile_frame[t] * kMaxCams + h_tile_cam[t];
    auto it = n_dropped_of.find(key);
    int nd = 0;
    if (it != n_dropped_of.end()) { nd = it->second; it->second = -1; }
    rows.push_back({h_tile_frame[t], h_tile_cam[t], h_tile_off[t + 1] - h_tile_off[t], marked[t] + nd, view[t], view[(size_t)std::max(T, 1) + t], worst[t]});
  }
  bool extra = false;
  for (const auto& kv : n_dropped_of)
    if (kv.second >= 0) { rows.push_back({(int)(kv.first / kMaxCams), (int)(kv.first % kMaxCams), 0, kv.second, 0.0, 0.0, -1}); extra = true; }
  if (extra) std::stable_sort(rows.begin(), rows.end(), [](const Row& a, const Row& b) { return a.frame != b.frame ? a.frame < b.frame : a.cam < b.cam; });
  const size_t V = rows.size();
  rep.v_frame.resize(V); rep.v_cam.resize(V); rep.v_count.resize(V); rep.v_removed.resize(V); rep.v_sq.resize(V); rep.v_max.resize(V); rep.v_worst.resize(V);
  for (size_t i = 0; i < V; ++i) {
    rep.v_frame[i] = rows[i].frame; rep.v_cam[i] = rows[i].cam; rep.v_count[i] = rows[i].count; rep.v_removed[i] = rows[i].removed;
    rep.v_sq[i] = rows[i].sq; rep.v_max[i] = rows[i].mx; rep.v_worst[i] = rows[i].worst;
  }
  (void)n_obs;
  rep.bins_x = bins_x; rep.bins_y = bins_y; rep.n_all = n_all; rep.last = r;
  rep.valid = true;
  return VC_OK;
}

#define NOT_RUNNING(h) do { if (!(h)) return VC_ERR_BAD_ARG; if ((h)->is_running) return VC_ERR_RUNNING; } while (0)
// a report can be read while it describes the problem and the state: computed, and nothing changed since
#define REPORT_READY(h) do { NOT_RUNNING(h); if (!(h)->rep.valid || (h)->device_dirty || (h)->rep.n_all != (h)->o_frame.size()) return VC_ERR_BAD_ARG; } while (0)

extern "C" {

int vc_report_compute(vc_calibrator* h, int bins_x, int bins_y) {
  NOT_RUNNING(h);
  if (bins_x < 1 || bins_x > 32 || bins_y < 1 || bins_y > 32) return VC_ERR_BAD_ARG;
  return h->report_compute(bins_x, bins_y);
}
long long vc_report_num_corners(vc_calibrator* h) {
  REPORT_READY(h);
  return (long long)h->rep.n_all;
}
int vc_report_corners(vc_calibrator* h, long long first, long long n, double* r, int* frame, int* camera, unsigned char* flags) {
  REPORT_READY(h);
  if (first < 0 || n < 0 || first + n > (long long)h->rep.n_all) return VC_ERR_BAD_ARG;
  for (long long i = 0; i < n; ++i) {
    const size_t k = (size_t)(first + i);
    if (frame) frame[i] = h->o_frame[k];
    if (camera) camera[i] = h->o_cam[k];
    if (flags) flags[i] = h->o_removed[k] == 1 ? 1 : (h->o_removed[k] == 2 ? 2 : 0);
  }
  if (!r || n == 0) return VC_OK;
  if (hipSetDevice(h->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  vc_calibrator::Report& rp = h->rep;
  if (!rp.stage && hipHostMalloc((void**)&rp.stage, vc_calibrator::Report::kStageCorners * sizeof(double2), hipHostMallocDefault) != hipSuccess) return VC_ERR_NO_DEVICE;
  for (long long done = 0; done < n;) {
    const size_t m = (size_t)std::min<long long>(n - done, (long long)vc_calibrator::Report::kStageCorners);
    if (hipMemcpyAsync(rp.stage, rp.d_res.p + first + done, m * sizeof(double2), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess) return VC_ERR_NO_DEVICE;
    std::memcpy(r + 2 * done, rp.stage, m * sizeof(double2));
    done += (long long)m;
  }
  return VC_OK;
}
int vc_report_num_views(vc_calibrator* h) {
  REPORT_READY(h);
  return (int)h->rep.v_frame.size();
}
int vc_report_views(vc_calibrator* h, int* frame, int* camera, int* count, int* removed, double* sum_sq, double* max_err, long long* worst_corner) {
  REPORT_READY(h);
  const vc_calibrator::Report& rp = h->rep;
  const size_t V = rp.v_frame.size();
  if (frame) std::memcpy(frame, rp.v_frame.data(), V * sizeof(int));
  if (camera) std::memcpy(camera, rp.v_cam.data(), V * sizeof(int));
  if (count) std::memcpy(count, rp.v_count.data(), V * sizeof(int));
  if (removed) std::memcpy(removed, rp.v_removed.data(), V * sizeof(int));
  if (sum_sq) std::memcpy(sum_sq, rp.v_sq.data(), V * sizeof(double));
  if (max_err) std::memcpy(max_err, rp.v_max.data(), V * sizeof(double));
  if (worst_corner) std::memcpy(worst_corner, rp.v_worst.data(), V * sizeof(long long));
  return VC_OK;
}
int vc_report_error_map(vc_calibrator* h, int camera, double* cells) {
  REPORT_READY(h);
  if (!cells || camera < 0 || camera >= (int)h->cams.size()) return VC_ERR_BAD_ARG;
  const size_t n = (size_t)h->rep.bins_x * h->rep.bins_y * 4;
  std::memcpy(cells, h->rep.map.data() + n * (size_t)camera, n * sizeof(double));
  return VC_OK;
}
int vc_report_num_imu_blocks(vc_calibrator* h) {
  REPORT_READY(h);
  return (int)h->rep.imu_flags.size();
}
int vc_report_imu(vc_calibrator* h, double* whitened, double* unwhitened, unsigned char* flags) {
  REPORT_READY(h);
  const vc_calibrator::Report& rp = h->rep;
  for (size_t s = 0; s < rp.imu_flags.size(); ++s) {
    if (whitened) std::memcpy(whitened + 9 * s, &rp.imu[s * kReportImuCols], 72);
    if (unwhitened) std::memcpy(unwhitened + 9 * s, &rp.imu[s * kReportImuCols + 9], 72);
    if (flags) flags[s] = (unsigned char)rp.imu_flags[s];
  }
  return VC_OK;
}

// Times the report's sweeps with HIP events on the calibrator's stream, `reps` launches each back to back (the results are rewritten
// with the same values): out_ms = vision sweep (+ dropped corners), error map (both passes), IMU sweep (k_imu_block + tail)
int vc_time_report_sweeps(vc_calibrator* h, int reps, double* out_ms) {
  REPORT_READY(h);
  if (!out_ms || reps < 1) return VC_ERR_BAD_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  EventSet<4> evs;
  if (!evs.create()) return VC_ERR_NO_DEVICE;
  const ReportView& r = h->rep.last;
  hipStream_t s = h->stream;
  for (int w = 0; w < 2; ++w) {      // first round warms clocks and caches
    (void)hipEventRecord(evs.e[0], s); for (int i = 0; i < reps; ++i) launch_report_vision(h->dv, r, s);
    (void)hipEventRecord(evs.e[1], s); for (int i = 0; i < reps; ++i) launch_report_map(h->dv, r, s);
    (void)hipEventRecord(evs.e[2], s); for (int i = 0; i < reps; ++i) if (r.n_blocks > 0) h->report_launch_imu(r);
    (void)hipEventRecord(evs.e[3], s);
    if (hipEventSynchronize(evs.e[3]) != hipSuccess) return VC_ERR_NO_DEVICE;
  }
  for (int i = 0; i < 3; ++i) { float ms = 0; (void)hipEventElapsedTime(&ms, evs.e[i], evs.e[i + 1]); out_ms[i] = ms / reps; }
  return VC_OK;
}

}  // extern "C"
