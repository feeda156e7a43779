// vck_util.hpp -- small utility kernels outside the pass: k_unpack, k_set_ctrl, k_reset_state, k_sum_tiles, k_cam_sq.
// (launch_unpack and launch_set_ctrl stand beside their kernels as they always did: moving them to the launchers would reorder the host code)
// Kernel fragment: defines __global__ symbols, so it belongs to exactly ONE translation unit -- vc_kernels.hip, which includes the
// fragments in stage order.  Not one of the VC_HD arithmetic headers (vc_math.hpp, ..): host harnesses cannot include it.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include "vc_math.hpp"
#include "vc_device.h"
#include "vc_kutil.hpp"

namespace vc {

// One stage's small uploads (vc_upload.cpp: upload): the host packs them into one page-locked staging image that goes to the
// device with ONE copy; this kernel scatters the image's segments to their buffers (several destinations may share a source: both
// state buffers and the "initial state" copy take the same poses) and zero-fills what a stage starts from zero.  Replaces ~45 small
// pageable copies / fills per stage (4.1 of the 19 ms of a complete cfg3 calibration).
__global__ __launch_bounds__(256) void k_unpack(const UnpackSeg* segs, int n, const unsigned* image) {
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nt = (size_t)gridDim.x * 256;
  for (int k = 0; k < n; ++k) {
    const UnpackSeg sg = segs[k];
    unsigned* dst = (unsigned*)sg.dst;
    const size_t words = sg.bytes >> 2;
    if (sg.src_off == ~0ull) { for (size_t i = tid; i < words; i += nt) dst[i] = 0u; }
    else { const unsigned* src = image + (sg.src_off >> 2); for (size_t i = tid; i < words; i += nt) dst[i] = src[i]; }
  }
}
void launch_unpack(const UnpackSeg* segs, int n, const void* image, size_t total_bytes, hipStream_t s) {
  const int blocks = (int)std::min<size_t>(512, std::max<size_t>(1, total_bytes / (256 * 16)));
  hipLaunchKernelGGL(k_unpack, dim3(blocks), dim3(256), 0, s, segs, n, (const unsigned*)image);
}
// a fresh control record for a solve: record 0 <- the host's (a kernel argument), record 1 blank -- one launch instead of a copy and a fill
__global__ __launch_bounds__(64) void k_set_ctrl(Ctrl* d, Ctrl c) {
  if (threadIdx.x == 0) { d[0] = c; Ctrl z = Ctrl(); d[1] = z; }
}
void launch_set_ctrl(Ctrl* d, const Ctrl& c, hipStream_t s) { hipLaunchKernelGGL(k_set_ctrl, dim3(1), dim3(64), 0, s, d, c); }
// both state buffers <- the uploaded initial state (benchmark restarts), one launch
__global__ __launch_bounds__(256) void k_reset_state(DevView v, const double* pose0, const double* cam0, const double* vel0, const double* imu0) {
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, n = (size_t)gridDim.x * 256;
  for (size_t i = tid; i < (size_t)v.n_frames * kPoseStride; i += n) { const double x = pose0[i]; v.poses[0][i] = x; v.poses[1][i] = x; }
  for (size_t i = tid; i < (size_t)v.n_cams * kCamStride; i += n) { const double x = cam0[i]; v.cams[0][i] = x; v.cams[1][i] = x; }
  for (size_t i = tid; i < (size_t)v.n_frames * 4; i += n) { const double x = vel0[i]; v.vel[0][i] = x; v.vel[1][i] = x; }
  for (size_t i = tid; i < 16; i += n) { const double x = imu0[i]; v.imus[0][i] = x; v.imus[1][i] = x; }
}

// out[0] = 1/2 sum tile_trial cost, out[1] = sum of squared residuals
__global__ __launch_bounds__(256) void k_sum_tiles(DevView v, double* out) {
  __shared__ double red[512];
  const int tid = threadIdx.x;
  double a = 0, b = 0;
  for (int t = tid; t < v.n_tiles; t += 256) { a += v.tile_trial[2 * t]; b += v.tile_trial[2 * t + 1]; }
  red[tid] = a; red[256 + tid] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (tid < o) { red[tid] += red[tid + o]; red[256 + tid] += red[256 + tid + o]; } __syncthreads(); }
  if (tid == 0) { out[0] = 0.5 * red[0]; out[1] = red[256]; }
}
// out[c*2] = sum of squared residuals of camera c, out[c*2+1] = corner count (per-camera RMSE, vicalibrator.h:958-971)
__global__ __launch_bounds__(256) void k_cam_sq(DevView v, double* out) {
  __shared__ double red[512];
  const int tid = threadIdx.x, c = blockIdx.x;
  double a = 0, b = 0;
  for (int t = tid; t < v.n_tiles; t += 256)
    if (v.tile_cam[t] == c) { a += v.tile_trial[2 * t + 1]; b += (double)(v.tile_off[t + 1] - v.tile_off[t]); }
  red[tid] = a; red[256 + tid] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (tid < o) { red[tid] += red[tid + o]; red[256 + tid] += red[256 + tid + o]; } __syncthreads(); }
  if (tid == 0) { out[c * 2] = red[0]; out[c * 2 + 1] = red[256]; }
}

}  // namespace vc
