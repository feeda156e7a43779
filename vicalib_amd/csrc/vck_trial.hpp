// vck_trial.hpp -- k_backsub, k_trial: the trial point of a vision-only pass.
// One wavefront per tile: back-substitution, T <- T exp(delta), trial residual sweep.
// Kernel fragment: defines __global__ symbols, so it belongs to exactly ONE translation unit -- vc_kernels.hip, which includes the
// fragments in stage order.  Not one of the VC_HD arithmetic headers (vc_math.hpp, ..): host harnesses cannot include it.
#pragma once
#include <hip/hip_runtime.h>
#include "vc_math.hpp"
#include "vc_device.h"
#include "vc_kutil.hpp"
#include "vck_reproj_jac.hpp"
#include "vck_reproj_res.hpp"

namespace vc {

// ------------------------------------------------------------------------------------------ trial point
// One wavefront per tile: delta_p = -L^-T (z + sum_tiles Y delta_s) (lanes = (tile, column), butterfly sum),
// T_trial = T exp(delta_p), residual sweep of the tile at the trial state.  The first tile of a frame
// also publishes the frame's trial pose and its step terms.
// Back-substitution of one frame: delta_p = -L^-T (z + sum_tiles Y delta_s) (lanes = (tile, column), six-value butterfly),
// T_trial = T exp(delta_p).  With `publish` lane 0 stores the trial pose and the frame's step terms (fpart).
__device__ __forceinline__ void backsub_frame(const DevView& v, int cur, int f, int lane, const double* ds_s, double* Tout, bool publish,
                                              double* wsum, const TileHdr* hdr = nullptr /* k_trial: the tile's header (registers) */) {
  const int t0 = hdr ? hdr->t0 : v.frame_tile_off[f], nt = hdr ? hdr->nt : v.frame_tile_off[f + 1] - t0;
  const double* fr = v.fr + (size_t)f * kFrStride;
  const double* pin = v.poses[cur] + (size_t)f * kPoseStride;
  double Lr[21], zr[6], di[6], Tin[7];
#pragma unroll
  for (int i = 0; i < 21; ++i) Lr[i] = fr[kFrL + i];
#pragma unroll
  for (int i = 0; i < 6; ++i) { zr[i] = fr[kFrZ + i]; di[i] = fr[kFrDinv + i]; }
#pragma unroll
  for (int i = 0; i < 7; ++i) Tin[i] = pin[i];
  double y[6] = {0, 0, 0, 0, 0, 0};
  const bool small_d = v.D <= kMaxCams * 16 + 16;
  for (int idx = lane; idx < nt * 16; idx += 64) {
    const int t = idx >> 4, j = idx & 15;
    if (hdr) {
      // columns and widths of the frame's tiles come with the header: the Y loads depend on nothing but t0 and go out
      // together with the frame record (Y's padding columns are zero and take a zero step)
      const int col0 = (int)((hdr->col0 >> (8 * t)) & 0xff), nc = (int)((hdr->ncols >> (8 * t)) & 0xff);
      const double* Yt = v.Y + (size_t)(t0 + t) * kYStride + j;
      double yv[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) yv[k] = Yt[k * kUCols];
      const int col = (j < nc) ? col0 + j : 0;
      double dj = small_d ? ds_s[col] : v.delta_s[col];
      dj = (j < nc) ? dj : 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) y[k] += yv[k] * dj;
    } else {
      const CamDesc cd = v.cd[v.tile_cam[t0 + t]];
      if (j < cd.ncols) {
        const double dj = small_d ? ds_s[cd.col0 + j] : v.delta_s[cd.col0 + j];
        const double* Yt = v.Y + (size_t)(t0 + t) * kYStride + j;
#pragma unroll
        for (int k = 0; k < 6; ++k) y[k] += Yt[k * kUCols] * dj;
      }
    }
  }
  double L[36];
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) L[i * 6 + j] = (j <= i) ? Lr[k++] : 0.0;
  }
  {
    double ys[6];
    wave_sum6(y, ys, lane);
#pragma unroll
    for (int k = 0; k < 6; ++k) y[k] = ys[k] + zr[k];
  }
  bwd_solve_inv<6>(L, di, y);
  double d[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) d[i] = -y[i];
  se3_plus(Tin, d, Tout);
  if (publish && lane == 0) {
    double* pout = v.poses[1 - cur] + (size_t)f * kPoseStride;
    double gd = 0, dld = 0, step2 = 0, x2 = 0, g2 = 0, gmax = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) { pout[i] = Tout[i]; const double e = Tout[i] - Tin[i]; step2 += e * e; x2 += Tin[i] * Tin[i]; }
    pout[7] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double gi = fr[kFrG + i];
      gd += gi * d[i]; dld += fr[kFrLam + i] * d[i] * d[i]; g2 += gi * gi; gmax = fmax(gmax, fabs(gi));
    }
    double* o = v.fpart + (size_t)f * kNumScal;
    o[kScGd] = gd; o[kScDld] = dld; o[kScStep2] = step2; o[kScX2] = x2; o[kScG2] = g2; o[kScCost] = 0.0; o[kScGmax] = gmax; o[kScSq] = 0.0;
    if (wsum) { wsum[kScGd] = gd; wsum[kScDld] = dld; wsum[kScStep2] = step2; wsum[kScX2] = x2; wsum[kScG2] = g2; wsum[kScGmax] = gmax; }
  }
}
// Large problems (more tiles than the chip holds waves): the back-substitution runs once per frame here instead of once
// per tile inside k_trial.
__global__ __launch_bounds__(256) void k_backsub(DevView v) {
  __shared__ double ds_s[kMaxCams * 16 + 16];
  const Ctrl* ct = v.ctrl;
  if (ct->done) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < v.D; i += 256) if (i < kMaxCams * 16 + 16) ds_s[i] = v.delta_s[i];
  __syncthreads();
  const int f = blockIdx.x * 4 + wave;
  if (f >= v.n_frames || v.frame_tile_off[f + 1] == v.frame_tile_off[f]) return;
  double Tout[7];
  backsub_frame(v, ct->cur, f, lane, ds_s, Tout, true, nullptr);
}
template <bool FUSED>
__device__ __forceinline__ void trial_tile(const DevView& v, int cur, double mult, TileHdr h, const double* cams_trial /* LDS */, int tile, int wave,
                                           int lane, const double* ds_s, double* lds_rows,
                                           double* wsum /* kNumScal, lane 0: this wave's step scalars */) {
  // the tile's header: one (wave-uniform) record instead of the chain tile -> frame -> frame's tiles -> cameras -> columns
  h.frame = __builtin_amdgcn_readfirstlane(h.frame); h.cam = __builtin_amdgcn_readfirstlane(h.cam);
  h.t0 = __builtin_amdgcn_readfirstlane(h.t0); h.nt = __builtin_amdgcn_readfirstlane(h.nt);
  h.off = __builtin_amdgcn_readfirstlane(h.off); h.cnt = __builtin_amdgcn_readfirstlane(h.cnt);
  h.model = __builtin_amdgcn_readfirstlane(h.model);
  const int f = h.frame, c = h.cam;
  const int t0 = h.t0;
  const double* cam = cams_trial + (size_t)c * kCamStride;
  double camr[kCamK + 10];
#pragma unroll
  for (int i = 0; i < kCamK + 10; ++i) camr[i] = cam[i];
  double Tout[7];
  if (v.pre_backsub) {            // k_backsub has been here: take the frame's trial pose and (first tile) its step terms
    const double* pt = v.poses[1 - cur] + (size_t)f * kPoseStride;
#pragma unroll
    for (int i = 0; i < 7; ++i) Tout[i] = pt[i];
    if (lane == 0 && tile == t0) {
      const double* o = v.fpart + (size_t)f * kNumScal;
      wsum[kScGd] = o[kScGd]; wsum[kScDld] = o[kScDld]; wsum[kScStep2] = o[kScStep2]; wsum[kScX2] = o[kScX2]; wsum[kScG2] = o[kScG2];
      wsum[kScGmax] = o[kScGmax];
    }
  } else {
    backsub_frame(v, cur, f, lane, ds_s, Tout, tile == t0, wsum, &h);
  }
  double cost, sq = 0.0;
  if (FUSED) {
    // Jacobian sweep at the trial point: its cost is the trial cost, its Gram block is the next linearisation if the
    // step is accepted (k_final flips `cur`); a rejected step leaves Gb[cur] untouched
    cost = jac_tile_dispatch(v, h.model, Tout, camr, mult, tile, lane, lds_rows + wave * 64 * kDotStride,
                             v.Gb[1 - cur] + (size_t)tile * kGPack, h.off, h.cnt);
    if (lane == 0) v.tile_costb[1 - cur][tile] = cost;
  } else {
    TileXf x;
    make_tile_xf(Tout, camr, &x);
    double K[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) K[i] = camr[kCamK + i];
    res_tile_dispatch(v, h.model, x, K, h.off, h.cnt, lane, mult, &cost, &sq);
  }
  if (lane == 0) {
    v.tile_trial[2 * tile] = cost;
    v.tile_trial[2 * tile + 1] = sq;
    wsum[kScCost] = cost;
  }
}
// (Tried and dropped: letting the last workgroup to finish run the final phase.  Device-scope release/acquire fences are
// expensive on this part -- every XCD has its own L2, so each fence writes back / invalidates L2 -- and cost 25 us at
// 250 workgroups; the kernel boundary does the same flush once.)
template <bool FUSED>
__global__ __launch_bounds__(256, 2) void k_trial(DevView v) {
  extern __shared__ __attribute__((aligned(16))) double lds_rows[];   // fused Jacobian sweep: 4 x 64 x kDotStride row images
  __shared__ double ds_s[kMaxCams * 16 + 16];     // delta_s of the workgroup's cameras is read many times: keep it in LDS
  __shared__ double s_cams[2 * kMaxCams * kCamStride];   // both camera buffers: requested before the control record says which is the trial one
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + wave;
  // everything that depends on nothing is requested first -- the tile's header, the shared step, the camera records --
  // then the control record; one memory latency instead of four in a row
  TileHdr h = v.tile_hdr[tile < v.n_tiles ? tile : 0];
  for (int i = threadIdx.x; i < v.D; i += 256) if (i < kMaxCams * 16 + 16) ds_s[i] = v.delta_s[i];
  for (int i = threadIdx.x; i < 2 * v.n_cams * kCamStride; i += 256) {
    const int b = i >= v.n_cams * kCamStride, o = i - b * v.n_cams * kCamStride;
    const double* src = b ? v.cams[1] : v.cams[0];
    s_cams[b * kMaxCams * kCamStride + o] = src[o];
  }
  const Ctrl* ct = v.ctrl;
  const int cur = ct->cur;
  const double mult = ct->mult;
  if (ct->done) return;
  __syncthreads();
  double wsum[kNumScal];
#pragma unroll
  for (int k = 0; k < kNumScal; ++k) wsum[k] = 0.0;
  if (tile < v.n_tiles) trial_tile<FUSED>(v, cur, mult, h, s_cams + (1 - cur) * kMaxCams * kCamStride, tile, wave, lane, ds_s, lds_rows, wsum);
  if (v.merged) {      // the workgroup's step scalars in one record: the next pass's decision reads n_tiles / 4 of these
    __shared__ double s_w[4 * kNumScal];
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < kNumScal; ++k) s_w[wave * kNumScal + k] = wsum[k];
    }
    __syncthreads();
    if (threadIdx.x < kNumScal) {
      const int k = threadIdx.x;
      const double a = s_w[k], b = s_w[kNumScal + k], c = s_w[2 * kNumScal + k], d = s_w[3 * kNumScal + k];
      v.wgpart[(size_t)blockIdx.x * kNumScal + k] = (k == kScGmax) ? fmax(fmax(a, b), fmax(c, d)) : (a + b) + (c + d);
    }
  }
}

}  // namespace vc
