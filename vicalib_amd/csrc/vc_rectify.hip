// vc_rectify.hip -- using the calibration of a PAIR: stereo rectification and the stereo consistency check (gfx950, wave64, fp64).
//
// A vc_rectifier holds two undistorters (vc_undistort.hip) that share one destination pinhole camera and whose rotations R_ds bring both
// cameras into a common frame in which a target point lies on the same image row and its depth is fu b / disparity (vc_rectify.hpp has
// the geometry).  Maps, images and points of either side are the undistorter's; what is new on the device is one sweep:
//
//   k_rectify_check   one wavefront per frame, four frames per 256-thread workgroup, built like k_validate_pose: no LDS, no block barrier,
//                     nothing shared between the waves of a workgroup.  Lanes stride over the frame's matched corner pairs.
//                     pass 1: both Newton inversions of a pair (undist_point), dv / d / P / v and a flag stored at the pair's place in the
//                             caller's order; per lane the sums of dv, dv^2, Z, P and X, the largest |dv| and the pair that has it.
//                     pass 2: the centred 3 x 3 cross-covariance sum (P - Pm)(X - Xm)^T; a lane re-reads the P it stored itself (a frame
//                             may have 32768 pairs: they do not stay in registers).
//                     pass 3: every lane solves the same 4 x 4 eigenproblem for the rotation (Horn's quaternion, cyclic Jacobi sweeps
//                             with compile-time indices: registers only, nothing depends on the lane).
//                     pass 4: the residuals sum |R (P - Pm) - (X - Xm)|^2 evaluated explicitly.
//                     Every reduction is the xor butterfly wave_allsum: a fixed order, the same bits in every lane, no floating-point
//                     atomic -- two runs, and a frame alone or among others, give the same bits.
// No CPU fallback: vc_rectifier_create fails with VC_ERR_NO_DEVICE without a HIP device.  vc_stereo_rectify_rotations,
// vc_stereo_fit_linear and vc_match_tiles are host code and need none.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <iterator>
#include <vector>
#include "../../include/vicalib_amd.h"
#include "vc_kutil.hpp"
#include "vc_hostutil.hpp"
#include "vc_rectify.hpp"

namespace {

using vc::RectPlan;
using vc::UndistPlan;
constexpr int kMaxFramePairs = 32768;
constexpr int kStatDoubles = 8;      // per frame: count, invalid, sum dv, sum dv^2, max |dv|, worst pair, mean Z, rigid rms

struct RectView {
  RectPlan plan;
  int n_frames;
  const long long* frame_off;        // n_frames + 1
  const double2* px_a; const double2* px_b;
  const double* target;              // n x 3 or nullptr
  double* pairs;                     // n x 6
  unsigned char* flags;              // n: 1 = invalid pair
  double* stats;                     // n_frames x kStatDoubles
};

__global__ __launch_bounds__(256) void k_rectify_check(RectView v) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + wave;
  if (f >= v.n_frames) return;                                 // (a whole wave leaves: nothing in this kernel waits for another wave)
  const long long o0 = v.frame_off[f];
  const int cnt = (int)(v.frame_off[f + 1] - o0);
  const double nan = __builtin_nan("");
  // ---- pass 1 --------------------------------------------------------------------------------------------------------------
  double s_dv = 0.0, s_dv2 = 0.0, s_z = 0.0, sp0 = 0.0, sp1 = 0.0, sp2 = 0.0, sx0 = 0.0, sx1 = 0.0, sx2 = 0.0, best = -1.0;
  long long best_i = -1;
  int nv = 0;
  for (int d = lane; d < cnt; d += 64) {                       // (ascending d = ascending caller index: ties keep the lowest)
    const long long i = o0 + d;
    const double2 a = v.px_a[i], b = v.px_b[i];
    double o[vc::kRectPairDoubles] = {nan, nan, nan, nan, nan, nan};
    const bool ok = vc::rectify_pair(v.plan, a.x, a.y, b.x, b.y, o);
    double* dst = v.pairs + vc::kRectPairDoubles * i;
#pragma unroll
    for (int k = 0; k < vc::kRectPairDoubles; ++k) dst[k] = o[k];
    v.flags[i] = ok ? 0 : 1;
    if (ok) {
      ++nv;
      s_dv += o[0]; s_dv2 += o[0] * o[0]; s_z += o[4];
      sp0 += o[2]; sp1 += o[3]; sp2 += o[4];
      if (v.target) { const double* X = v.target + 3 * i; sx0 += X[0]; sx1 += X[1]; sx2 += X[2]; }
      const double e = fabs(o[0]);
      if (e > best) { best = e; best_i = i; }
    }
  }
  nv = vc::wave_allsum(nv);
  s_dv = vc::wave_allsum(s_dv); s_dv2 = vc::wave_allsum(s_dv2); s_z = vc::wave_allsum(s_z);
  vc::wave_argmax_low(&best, &best_i);                         // the same pair in every lane: larger |dv|, then the lower index
  // ---- passes 2 - 4: the rigid fit of the triangulated corners onto the target (rotation + translation, NO scale) ------------------
  double rms = nan;
  if (v.target && nv >= 3) {                                   // (wave-uniform: nv is the same in every lane)
    const double inv = 1.0 / (double)nv;
    const double Pm[3] = {vc::wave_allsum(sp0) * inv, vc::wave_allsum(sp1) * inv, vc::wave_allsum(sp2) * inv};
    const double Xm[3] = {vc::wave_allsum(sx0) * inv, vc::wave_allsum(sx1) * inv, vc::wave_allsum(sx2) * inv};
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int d = lane; d < cnt; d += 64) {
      const long long i = o0 + d;
      if (v.flags[i]) continue;
      const double* P = v.pairs + vc::kRectPairDoubles * i + 2;
      const double* X = v.target + 3 * i;
      const double p[3] = {P[0] - Pm[0], P[1] - Pm[1], P[2] - Pm[2]}, x[3] = {X[0] - Xm[0], X[1] - Xm[1], X[2] - Xm[2]};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) H[3 * r + c] += p[r] * x[c];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] = vc::wave_allsum(H[k]);
    double R[9];
    vc::rigid_rotation(H, R);
    double ss = 0.0;
    for (int d = lane; d < cnt; d += 64) {
      const long long i = o0 + d;
      if (v.flags[i]) continue;
      ss += vc::rigid_residual_sq(R, v.pairs + vc::kRectPairDoubles * i + 2, Pm, v.target + 3 * i, Xm);
    }
    rms = sqrt(vc::wave_allsum(ss) * inv);
  }
  if (lane == 0) {
    double* s = v.stats + (size_t)f * kStatDoubles;
    s[0] = (double)nv; s[1] = (double)(cnt - nv); s[2] = s_dv; s[3] = s_dv2; s[4] = best_i >= 0 ? best : 0.0; s[5] = (double)best_i;
    s[6] = nv > 0 ? s_z / (double)nv : 0.0; s[7] = rms;
  }
}

// Shepperd: the unit quaternion [x y z w] of a rotation matrix (row-major)
void quat_from_R(const double* R, double* q) {
  const double tr = R[0] + R[4] + R[8];
  if (tr > 0.0) {
    const double s = 2.0 * std::sqrt(tr + 1.0);
    q[3] = 0.25 * s; q[0] = (R[7] - R[5]) / s; q[1] = (R[2] - R[6]) / s; q[2] = (R[3] - R[1]) / s;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const double s = 2.0 * std::sqrt(1.0 + R[0] - R[4] - R[8]);
    q[3] = (R[7] - R[5]) / s; q[0] = 0.25 * s; q[1] = (R[1] + R[3]) / s; q[2] = (R[2] + R[6]) / s;
  } else if (R[4] > R[8]) {
    const double s = 2.0 * std::sqrt(1.0 + R[4] - R[0] - R[8]);
    q[3] = (R[2] - R[6]) / s; q[0] = (R[1] + R[3]) / s; q[1] = 0.25 * s; q[2] = (R[5] + R[7]) / s;
  } else {
    const double s = 2.0 * std::sqrt(1.0 + R[8] - R[0] - R[4]);
    q[3] = (R[3] - R[1]) / s; q[0] = (R[2] + R[6]) / s; q[1] = (R[5] + R[7]) / s; q[2] = 0.25 * s;
  }
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int k = 0; k < 4; ++k) q[k] /= n;
}
using vc::pose_ok;
int rotation_status(int rc) { return rc == vc::kRectOk ? VC_OK : rc == vc::kRectCoincident ? VC_ERR_NUMERIC : VC_ERR_UNSUPPORTED; }

}  // namespace

struct vc_rectifier {
  int device = 0;
  vc_undistorter* side[2] = {nullptr, nullptr};
  RectPlan plan;
  double R_ds[2][9];
  double T_rect[2][7];
  hipStream_t stream = nullptr;      // side a's: the check runs there
  // the check's device buffers: [frame_off | px_a | px_b | target | pairs | flags | stats], grown to the largest problem seen
  unsigned char* d_buf = nullptr;
  size_t cap_pairs = 0, cap_frames = 0;
  RectView last;                     // the last check's launch, for vc_time_rectify_check
  bool have_last = false, in_flight = false;
};

namespace {

void carve_check(vch::Carver* c, size_t cp, size_t cf, RectView* v) {
  v->frame_off = c->take<long long>(cf + 1);
  v->px_a = c->take<double2>(cp); v->px_b = c->take<double2>(cp);
  v->target = c->take<double>(cp * 3);
  v->pairs = c->take<double>(cp * vc::kRectPairDoubles);
  v->flags = c->take<unsigned char>(cp);
  v->stats = c->take<double>(cf * kStatDoubles);
}
bool reserve_check(vc_rectifier* r, size_t n, size_t nf, RectView* v) {
  if (n > r->cap_pairs || nf > r->cap_frames) {
    const size_t cp = std::max(n, r->cap_pairs), cf = std::max(nf, r->cap_frames);
    (void)hipStreamSynchronize(r->stream);
    (void)hipFree(r->d_buf); r->d_buf = nullptr; r->cap_pairs = r->cap_frames = 0; r->have_last = false;
    vch::Carver size;
    carve_check(&size, cp, cf, v);
    if (hipMalloc((void**)&r->d_buf, size.bytes()) != hipSuccess) return false;
    r->cap_pairs = cp; r->cap_frames = cf;
  }
  vch::Carver at(r->d_buf);
  carve_check(&at, r->cap_pairs, r->cap_frames, v);
  return true;
}
void launch_check(vc_rectifier* r, const RectView& v) {
  hipLaunchKernelGGL(k_rectify_check, dim3((v.n_frames + 3) / 4), dim3(256), 0, r->stream, v);
}

}  // namespace

extern "C" {

int vc_stereo_rectify_rotations(const double T_ck_a[7], const double T_ck_b[7], double R_ds_a[9], double R_ds_b[9], double* baseline) {
  double Ta[7], Tb[7], Ra[9], Rb[9], b = 0.0;
  if (!pose_ok(T_ck_a, Ta) || !pose_ok(T_ck_b, Tb)) return VC_ERR_BAD_ARG;
  const int rc = rotation_status(vc::rectify_rotations(Ta, Tb, Ra, Rb, &b));
  if (rc != VC_OK) return rc;
  if (R_ds_a) std::memcpy(R_ds_a, Ra, 72);
  if (R_ds_b) std::memcpy(R_ds_b, Rb, 72);
  if (baseline) *baseline = b;
  return VC_OK;
}

int vc_stereo_fit_linear(int model_a, const double* params_a, int nparams_a, int w_a, int h_a, const double R_ds_a[9], int model_b, const double* params_b,
                         int nparams_b, int w_b, int h_b, const double R_ds_b[9], int dst_w, int dst_h, double alpha, double dst_linear[4]) {
  if (!vc::undist_source_args_ok(model_a, params_a, nparams_a, w_a, h_a) || !vc::undist_source_args_ok(model_b, params_b, nparams_b, w_b, h_b)) return VC_ERR_BAD_ARG;
  if (!dst_linear || !vc::undist_dest_args_ok(nullptr, dst_w, dst_h, 0) || !(alpha >= 0.0 && alpha <= 1.0)) return VC_ERR_BAD_ARG;
  UndistPlan side[2];
  vc::undist_source_plan(&side[0], model_a, params_a, nparams_a, w_a, h_a, R_ds_a);
  vc::undist_source_plan(&side[1], model_b, params_b, nparams_b, w_b, h_b, R_ds_b);
  return vc::undist_fit_sides(2, side, dst_w, dst_h, alpha, dst_linear);
}

int vc_match_tiles(int n_tiles, const int* tile_frame, const int* tile_cam, const long long* tile_off, const int* point_id, int cam_a, int cam_b,
                   int* n_frames, long long* n_pairs, int* frame, long long* frame_off, long long* pos_a, long long* pos_b) {
  if (n_tiles < 0 || (n_tiles > 0 && (!tile_frame || !tile_cam || !tile_off || !point_id)) || cam_a < 0 || cam_b < 0 || cam_a == cam_b || !n_frames || !n_pairs)
    return VC_ERR_BAD_ARG;
  const bool fill = frame || frame_off || pos_a || pos_b;
  if (fill && (!frame_off || !pos_a || !pos_b)) return VC_ERR_BAD_ARG;
  for (int t = 0; t < n_tiles; ++t) if (tile_off[t + 1] < tile_off[t] || tile_frame[t] < 0) return VC_ERR_BAD_ARG;
  struct Corner { int frame, id; long long pos; };
  std::vector<Corner> c[2];
  std::vector<int> seen[2];                                // frames a side has a tile of (corners or not)
  for (int t = 0; t < n_tiles; ++t) {
    const int s = tile_cam[t] == cam_a ? 0 : tile_cam[t] == cam_b ? 1 : -1;
    if (s < 0) continue;
    seen[s].push_back(tile_frame[t]);
    for (long long k = tile_off[t]; k < tile_off[t + 1]; ++k) c[s].push_back({tile_frame[t], point_id[k], k});
  }
  for (int s = 0; s < 2; ++s) {
    std::sort(seen[s].begin(), seen[s].end());
    seen[s].erase(std::unique(seen[s].begin(), seen[s].end()), seen[s].end());
    // by frame, then point id, then position: of a point id given twice in one view the first position counts
    std::sort(c[s].begin(), c[s].end(), [](const Corner& x, const Corner& y) { return x.frame != y.frame ? x.frame < y.frame : x.id != y.id ? x.id < y.id : x.pos < y.pos; });
    c[s].erase(std::unique(c[s].begin(), c[s].end(), [](const Corner& x, const Corner& y) { return x.frame == y.frame && x.id == y.id; }), c[s].end());
  }
  std::vector<int> both;
  std::set_intersection(seen[0].begin(), seen[0].end(), seen[1].begin(), seen[1].end(), std::back_inserter(both));
  const int cap_f = *n_frames; const long long cap_p = *n_pairs;
  long long np = 0;
  size_t ia = 0, ib = 0;
  for (size_t k = 0; k < both.size(); ++k) {
    const int f = both[k];
    if (fill && (int)k < cap_f) { if (frame) frame[k] = f; frame_off[k] = np; }
    while (ia < c[0].size() && c[0][ia].frame < f) ++ia;
    while (ib < c[1].size() && c[1][ib].frame < f) ++ib;
    while (ia < c[0].size() && ib < c[1].size() && c[0][ia].frame == f && c[1][ib].frame == f) {
      if (c[0][ia].id < c[1][ib].id) ++ia;
      else if (c[1][ib].id < c[0][ia].id) ++ib;
      else {
        if (fill && np < cap_p) { pos_a[np] = c[0][ia].pos; pos_b[np] = c[1][ib].pos; }
        ++np; ++ia; ++ib;
      }
    }
  }
  *n_frames = (int)both.size(); *n_pairs = np;
  if (fill) {
    if ((int)both.size() > cap_f || np > cap_p) return VC_ERR_BAD_ARG;
    frame_off[both.size()] = np;
  }
  return VC_OK;
}

int vc_rectifier_create(int device, int model_a, const double* params_a, int nparams_a, int w_a, int h_a, const double T_ck_a[7], int model_b,
                        const double* params_b, int nparams_b, int w_b, int h_b, const double T_ck_b[7], const double dst_linear[4], int dst_w, int dst_h,
                        double alpha, int fill, vc_rectifier** out) {
  double Ta[7], Tb[7];
  if (!out || !vc::undist_source_args_ok(model_a, params_a, nparams_a, w_a, h_a) || !vc::undist_source_args_ok(model_b, params_b, nparams_b, w_b, h_b)) return VC_ERR_BAD_ARG;
  if (!vc::undist_dest_args_ok(dst_linear, dst_w, dst_h, fill) || !pose_ok(T_ck_a, Ta) || !pose_ok(T_ck_b, Tb)) return VC_ERR_BAD_ARG;
  if (!dst_linear && !(alpha >= 0.0 && alpha <= 1.0)) return VC_ERR_BAD_ARG;
  vc_rectifier* r = new vc_rectifier;
  std::memset(&r->plan, 0, sizeof(r->plan)); std::memset(&r->last, 0, sizeof(r->last));
  int rc = rotation_status(vc::rectify_rotations(Ta, Tb, r->R_ds[0], r->R_ds[1], &r->plan.baseline));
  double dl[4];
  if (rc == VC_OK) {
    if (dst_linear) std::memcpy(dl, dst_linear, 32);
    else rc = vc_stereo_fit_linear(model_a, params_a, nparams_a, w_a, h_a, r->R_ds[0], model_b, params_b, nparams_b, w_b, h_b, r->R_ds[1], dst_w, dst_h, alpha, dl);
  }
  if (rc == VC_OK) rc = vc_undistorter_create(device, model_a, params_a, nparams_a, w_a, h_a, dl, dst_w, dst_h, r->R_ds[0], fill, &r->side[0]);
  if (rc == VC_OK) rc = vc_undistorter_create(device, model_b, params_b, nparams_b, w_b, h_b, dl, dst_w, dst_h, r->R_ds[1], fill, &r->side[1]);
  if (rc != VC_OK) { vc_rectifier_destroy(r); return rc; }
  r->device = device;
  r->plan.a = vc::undist_plan_of(r->side[0]); r->plan.b = vc::undist_plan_of(r->side[1]);
  r->stream = (hipStream_t)vc_undistort_stream(r->side[0]);
  const double* T[2] = {Ta, Tb};
  for (int s = 0; s < 2; ++s) {                        // T_ck_rect = (R_ds R_ck, R_ds t_ck)
    double Rck[9], Rr[9];
    vc::quat_to_R(T[s], Rck);
    const double* D = r->R_ds[s];
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) Rr[3 * i + j] = D[3 * i] * Rck[j] + D[3 * i + 1] * Rck[3 + j] + D[3 * i + 2] * Rck[6 + j];
      r->T_rect[s][4 + i] = D[3 * i] * T[s][4] + D[3 * i + 1] * T[s][5] + D[3 * i + 2] * T[s][6];
    }
    quat_from_R(Rr, r->T_rect[s]);
  }
  *out = r;
  return VC_OK;
}
void vc_rectifier_destroy(vc_rectifier* r) {
  if (!r) return;
  if (r->stream) { (void)hipSetDevice(r->device); (void)hipStreamSynchronize(r->stream); }
  if (r->d_buf) (void)hipFree(r->d_buf);
  vc_undistorter_destroy(r->side[0]); vc_undistorter_destroy(r->side[1]);
  delete r;
}
vc_undistorter* vc_rectifier_side(vc_rectifier* r, int side) { return (r && (side == 0 || side == 1)) ? r->side[side] : nullptr; }

int vc_rectifier_get(vc_rectifier* r, double R_ds_a[9], double R_ds_b[9], double dst_linear[4], int dst_size[2], double* baseline, double T_ck_rect_a[7],
                     double T_ck_rect_b[7]) {
  if (!r) return VC_ERR_BAD_ARG;
  if (R_ds_a) std::memcpy(R_ds_a, r->R_ds[0], 72);
  if (R_ds_b) std::memcpy(R_ds_b, r->R_ds[1], 72);
  if (dst_linear) std::memcpy(dst_linear, r->plan.a.dl, 32);
  if (dst_size) { dst_size[0] = r->plan.a.dst_w; dst_size[1] = r->plan.a.dst_h; }
  if (baseline) *baseline = r->plan.baseline;
  if (T_ck_rect_a) std::memcpy(T_ck_rect_a, r->T_rect[0], 56);
  if (T_ck_rect_b) std::memcpy(T_ck_rect_b, r->T_rect[1], 56);
  return VC_OK;
}

int vc_rectify_pairs(vc_rectifier* r, int n, const unsigned char* src_a, int src_pitch_a, long long src_stride_a, const unsigned char* src_b, int src_pitch_b,
                     long long src_stride_b, unsigned char* dst_a, int dst_pitch_a, long long dst_stride_a, unsigned char* dst_b, int dst_pitch_b,
                     long long dst_stride_b) {
  if (!r) return VC_ERR_BAD_ARG;
  // both sides' uploads, remaps and downloads are enqueued on their own streams before either is waited for
  int rc = vc::undist_images_begin(r->side[0], n, src_a, src_pitch_a, src_stride_a, dst_a, dst_pitch_a, dst_stride_a);
  if (rc != VC_OK) return rc;
  rc = vc::undist_images_begin(r->side[1], n, src_b, src_pitch_b, src_stride_b, dst_b, dst_pitch_b, dst_stride_b);
  const int ra = vc::undist_images_end(r->side[0], n, dst_a, dst_pitch_a, dst_stride_a);      // (side a is always finished, whatever b's begin said)
  if (rc != VC_OK) return rc;
  const int rb = vc::undist_images_end(r->side[1], n, dst_b, dst_pitch_b, dst_stride_b);
  return ra != VC_OK ? ra : rb;
}

int vc_rectify_check(vc_rectifier* r, int n_frames, const long long* frame_off, const double* px_a, const double* px_b, const double* target, double* pairs_out,
                     unsigned char* flags, int* count, int* invalid, double* sum_dv, double* sum_dv2, double* max_abs_dv, long long* worst, double* mean_z,
                     double* rigid_rms) {
  if (!r || n_frames < 0 || (n_frames > 0 && !frame_off)) return VC_ERR_BAD_ARG;
  if (n_frames == 0) return VC_OK;
  if (frame_off[0] != 0) return VC_ERR_BAD_ARG;
  for (int f = 0; f < n_frames; ++f) if (frame_off[f + 1] < frame_off[f] || frame_off[f + 1] - frame_off[f] > kMaxFramePairs) return VC_ERR_BAD_ARG;
  const size_t n = (size_t)frame_off[n_frames];
  if (n > 0 && (!px_a || !px_b)) return VC_ERR_BAD_ARG;
  if (hipSetDevice(r->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  if (r->in_flight) (void)hipStreamSynchronize(r->stream);
  RectView v;
  v.plan = r->plan; v.n_frames = n_frames;
  if (!reserve_check(r, n, (size_t)n_frames, &v)) return VC_ERR_NO_DEVICE;
  r->in_flight = true; r->have_last = false;
  hipStream_t s = r->stream;
  bool ok = hipMemcpyAsync((void*)v.frame_off, frame_off, ((size_t)n_frames + 1) * 8, hipMemcpyHostToDevice, s) == hipSuccess;
  if (n > 0) {
    ok = ok && hipMemcpyAsync((void*)v.px_a, px_a, n * 16, hipMemcpyHostToDevice, s) == hipSuccess && hipMemcpyAsync((void*)v.px_b, px_b, n * 16, hipMemcpyHostToDevice, s) == hipSuccess;
    if (target) ok = ok && hipMemcpyAsync((void*)v.target, target, n * 24, hipMemcpyHostToDevice, s) == hipSuccess;
  }
  if (!target) v.target = nullptr;
  if (!ok) return VC_ERR_NO_DEVICE;
  launch_check(r, v);
  std::vector<double> st((size_t)n_frames * kStatDoubles);
  ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(st.data(), v.stats, st.size() * 8, hipMemcpyDeviceToHost, s) == hipSuccess;
  if (n > 0 && pairs_out) ok = ok && hipMemcpyAsync(pairs_out, v.pairs, n * 48, hipMemcpyDeviceToHost, s) == hipSuccess;
  if (n > 0 && flags) ok = ok && hipMemcpyAsync(flags, v.flags, n, hipMemcpyDeviceToHost, s) == hipSuccess;
  if (!ok || hipStreamSynchronize(s) != hipSuccess) return VC_ERR_NO_DEVICE;
  r->in_flight = false;
  r->last = v; r->have_last = true;
  for (int f = 0; f < n_frames; ++f) {
    const double* q = st.data() + (size_t)f * kStatDoubles;
    if (count) count[f] = (int)q[0];
    if (invalid) invalid[f] = (int)q[1];
    if (sum_dv) sum_dv[f] = q[2];
    if (sum_dv2) sum_dv2[f] = q[3];
    if (max_abs_dv) max_abs_dv[f] = q[4];
    if (worst) worst[f] = (long long)q[5];
    if (mean_z) mean_z[f] = q[6];
    if (rigid_rms) rigid_rms[f] = q[7];
  }
  return VC_OK;
}

int vc_time_rectify_check(vc_rectifier* r, int reps, double* out_ms) {
  if (!r || reps < 1 || !out_ms || !r->have_last) return VC_ERR_BAD_ARG;
  if (hipSetDevice(r->device) != hipSuccess) return VC_ERR_NO_DEVICE;
  return vch::time_back_to_back(r->stream, reps, [&]() { launch_check(r, r->last); }, out_ms);      // (a launch rewrites the same results)
}

}  // extern "C"
