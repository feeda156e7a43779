// vck_reproj_res.hpp -- k_reproj_res, k_outlier_mask: plain residual sweeps of one state buffer (RMSE, the outlier mask).
// Kernel fragment: defines __global__ symbols, so it belongs to exactly ONE translation unit -- vc_kernels.hip, which includes the
// fragments in stage order.  Not one of the VC_HD arithmetic headers (vc_math.hpp, ..): host harnesses cannot include it.
#pragma once
#include <hip/hip_runtime.h>
#include "vc_math.hpp"
#include "vc_device.h"
#include "vc_kutil.hpp"

namespace vc {

// ------------------------------------------------------------------------------------------ residual sweeps
template <int MODEL>
__device__ __forceinline__ void res_tile_sweep(const DevView& v, const TileXf& x, const double* K, int off, int cnt, int lane,
                                               double mult, double* cost_out, double* sq_out) {
  double cost = 0.0, sq = 0.0;
  ModelPre pre;
  model_precompute(MODEL, K, &pre);
  for (int d = lane; d < cnt; d += 64) {
    const double2 uv = v.obs_uv[off + d];
    const int id = v.obs_pt[off + d];
    const double* pw = v.points + 3 * (size_t)(id & kObsPointMask);
    double r[2];
    cost += ((id & kObsOneLess) ? mult - 1.0 : mult) * corner_residual<MODEL>(x, K, pre, pw, uv.x, uv.y, r);
    sq += r[0] * r[0] + r[1] * r[1];
  }
  *cost_out = wave_sum(cost);
  *sq_out = wave_sum(sq);
}
__device__ __forceinline__ void res_tile_dispatch(const DevView& v, int model, const TileXf& x, const double* K, int off, int cnt,
                                                  int lane, double mult, double* cost, double* sq) {
  with_model(model, [&](auto m) { res_tile_sweep<decltype(m)::value>(v, x, K, off, cnt, lane, mult, cost, sq); });
}
// plain sweep of one state buffer (RMSE, vc_evaluate): tile_trial[t] = {mult * sum rho, sum |r|^2}
__global__ __launch_bounds__(256) void k_reproj_res(DevView v, int state, double mult) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + wave;
  if (tile >= v.n_tiles) return;
  if (state >= 2) {            // 2: accepted buffer, 3: trial buffer of the running solve (multiplicity from Ctrl)
    const Ctrl* ct = v.ctrl;
    if (ct->done) return;
    state = (state == 3) ? 1 - ct->cur : ct->cur;
    mult = ct->mult;
  }
  const int f = v.tile_frame[tile], c = v.tile_cam[tile];
  TileXf x;
  double K[10];
  view_setup(v.poses[state] + (size_t)f * kPoseStride, v.cams[state] + (size_t)c * kCamStride, &x, K);
  double cost, sq;
  res_tile_dispatch(v, v.cd[c].model, x, K, v.tile_off[tile], v.tile_off[tile + 1] - v.tile_off[tile], lane, mult, &cost, &sq);
  if (lane == 0) { v.tile_trial[2 * tile] = cost; v.tile_trial[2 * tile + 1] = sq; }
}

// per-corner outlier mask (RemoveOutliers, vicalibrator.h:859-916): |r| > thresh[cam]
template <int MODEL>
__device__ __forceinline__ void mask_tile_body(const DevView& v, const TileXf& x, const double* K, int off, int cnt, int lane,
                                               double th, unsigned char* mask) {
  ModelPre pre;
  model_precompute(MODEL, K, &pre);
  for (int d = lane; d < cnt; d += 64) {
    const double2 uv = v.obs_uv[off + d];
    double r[2];
    corner_residual<MODEL>(x, K, pre, v.points + 3 * (size_t)(v.obs_pt[off + d] & kObsPointMask), uv.x, uv.y, r);
    mask[off + d] = sqrt(r[0] * r[0] + r[1] * r[1]) > th ? 1 : 0;
  }
}
__global__ __launch_bounds__(256) void k_outlier_mask(DevView v, int state, const double* thresh, unsigned char* mask) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + wave;
  if (tile >= v.n_tiles) return;
  const int f = v.tile_frame[tile], c = v.tile_cam[tile];
  const int off = v.tile_off[tile], cnt = v.tile_off[tile + 1] - off;
  TileXf x;
  double K[10];
  view_setup(v.poses[state] + (size_t)f * kPoseStride, v.cams[state] + (size_t)c * kCamStride, &x, K);
  const double th = thresh[c];
  with_model(v.cd[c].model, [&](auto m) { mask_tile_body<decltype(m)::value>(v, x, K, off, cnt, lane, th, mask); });
}

}  // namespace vc
