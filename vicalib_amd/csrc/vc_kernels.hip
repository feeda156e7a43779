// vc_kernels.hip -- CDNA4 (gfx950, wave64) kernels of the batched Levenberg-Marquardt engine.
//
// Replaces, on the device, what the reference does per residual block inside ceres::Solve
// (vicalibrator.h:956): AutoDiffCostFunction::Evaluate of ImuReprojectionCostFunctor
// (ceres-cost-functions.h:350-373) + loss correction + block-sparse J^T J, the elimination of the
// per-frame pose blocks (Ceres' sparse Cholesky), the dense solve on the shared parameters, the
// manifold update (local-param-se3.h), the cost evaluation of the trial point and the trust-region
// bookkeeping (step quality, radius, termination tests, iteration callback vicalibrator.h:690-721).
//
// This file is the stage index: the kernels stand in the fragments below (vck_*.hpp, one per stage, each with its own description), included
// in the order of a pass; the launchers follow.  The fragments define __global__ symbols and belong to this translation unit alone.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "vc_math.hpp"
#include "vc_device.h"
#include "vc_kutil.hpp"

// (the order is part of the build: a device function that is not __forceinline__ must stay ahead of its callers)
#include "vck_reproj_jac.hpp"   // jac_tile_body, jac_tile_body_split, k_reproj_jac
#include "vck_reproj_res.hpp"   // k_reproj_res, k_outlier_mask
#include "vck_frame_schur.hpp"  // k_frame_schur, part_sum_block, k_part_sum
#include "vck_reduced.hpp"      // schur_final_phase, solve_small_wave, factor / solve_large_tiled, k_reduced
#include "vck_trial.hpp"        // backsub_frame, k_backsub, trial_tile, k_trial
#include "vck_decide.hpp"       // lm_decide*, merged_control, k_final_merged, final_phase*, k_wait_flag, k_signal_flag, k_final
#include "vck_util.hpp"         // k_unpack, k_set_ctrl, k_reset_state, k_sum_tiles, k_cam_sq

namespace vc {

// ------------------------------------------------------------------------------------------ launchers
static inline int tiles_grid(const DevView& v) { return (v.n_tiles + 3) / 4; }

void launch_reproj_jac(const DevView& v, hipStream_t s, int trial) {
  if (v.n_tiles == 0) return;
  // (one workgroup per CU for the visual-inertial trial sweep, so that k_imu_jac(trial) shares every SIMD with it from the start, was
  //  measured slower: 0.2075 against 0.2035 ms per iteration)
  const size_t lds = 4 * 64 * kDotStride * sizeof(double);
  hipLaunchKernelGGL(k_reproj_jac, dim3(tiles_grid(v)), dim3(256), lds, s, v, trial);
}
void launch_part_sum(const DevView& v, hipStream_t s) {
  // (hadd_early: the entries behind S and g_red were summed ahead of this launch, vc_shared_blocks.hpp -- only the frames' partial sums are left)
  const int entries = v.hadd_early ? v.D * v.D + v.D : v.part_stride;
  hipLaunchKernelGGL(k_part_sum, dim3((entries + kSumEntries - 1) / kSumEntries), dim3(kSumEntries * kSumSlices), 0, s, v);
}
void launch_frame_schur(const DevView& v, hipStream_t s) {
  const int D = v.D;
  const int Dp = ((D + 1 + 15) / 16) * 16, ld = (Dp % 32 == 0) ? Dp + 16 : Dp;
  const size_t lds = ((size_t)4 * (v.n_cams * kGStride + kPrepPad) + (size_t)24 * ld) * sizeof(double);
  const int nT = (D + 1 + 15) / 16;
  auto go = [&](auto kern) {
    if (lds > 65536) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3(v.n_chunks), dim3(256), lds, s, v);
  };
  if (v.n_cams <= 2 && nT <= 2) go(k_frame_schur<2, 1, 2>);
  else if (v.n_cams <= 4 && nT <= 4) go(k_frame_schur<4, 3, 2>);
  else go(k_frame_schur<kMaxCams, kMaxPairsPerWave, 2>);
  launch_part_sum(v, s);
}
static inline size_t reduced_lds(const DevView& v) {
  const size_t solve = v.D <= kSmallD ? ((size_t)(kSmallD + 1) * (kSmallD + 2) + 3 * (kSmallD + 1)) * sizeof(double)
                                      : ((size_t)(v.D + 1) * (v.D + 2) / 2 + 3 * (v.D + 1) + 2 + 384 + 384) * sizeof(double);      // (M, row D, x, dinv; two column images)
  const size_t top = (v.gram_top_stride > 0 && v.D <= kEarlyTopD) ? (size_t)64 * kTopLd * sizeof(double) : 0;      // (k_reduced: s_top)
  return std::max(solve, (sizeof(FinalLds) + 7) / 8 * 8 + top);
}
// the reduced system's LDS image fits the workgroup's 160 KB (k_reduced: static tables + the packed triangle): D <= 179 on gfx950 -- BASELINE
// cfg5 over 8 ranks is D = 178.  Asked of the runtime, not assumed: a launch beyond it fails without a word.
bool reduced_fits(const DevView& v) {
  hipFuncAttributes fa;
  int dev = 0, max_lds = 0;
  if (hipFuncGetAttributes(&fa, (const void*)k_reduced) != hipSuccess || hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) { (void)hipGetLastError(); return true; }
  if (max_lds < 163840) max_lds = 163840;      // (gfx950: 160 KB per workgroup once hipFuncAttributeMaxDynamicSharedMemorySize is granted; the attribute reports the default 64 KB)
  return reduced_lds(v) + fa.sharedSizeBytes <= (size_t)max_lds;
}
void launch_reduced(const DevView& v, int mode, hipStream_t s) {
  const size_t lds = reduced_lds(v);
  static LdsGrant granted;
  if (lds > 30000 && granted.need(lds)) (void)hipFuncSetAttribute((const void*)k_reduced, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k_reduced, dim3(1), dim3(256), lds, s, v, mode);
}
void launch_trial(const DevView& v, hipStream_t s) {
  if (v.n_tiles == 0) return;
  if (v.pre_backsub) hipLaunchKernelGGL(k_backsub, dim3((v.n_frames + 3) / 4), dim3(256), 0, s, v);
  const size_t lds = 4 * 64 * kDotStride * sizeof(double);
  static LdsGrant granted;
  if (lds > 0 && granted.need(lds + 4096)) (void)hipFuncSetAttribute((const void*)k_trial<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds + 4096));
  hipLaunchKernelGGL(k_trial<true>, dim3(tiles_grid(v)), dim3(256), lds, s, v);      // vision-only passes are always fused
}
void launch_final_merged(const DevView& v, hipStream_t s) { hipLaunchKernelGGL(k_final_merged, dim3(1), dim3(256), 0, s, v); }
void launch_final(const DevView& v, int mode, hipStream_t s) {
  hipLaunchKernelGGL(k_final, dim3(1), dim3(256), 0, s, v, mode);
}
void launch_wait_flag(const DevView& v, int idx, long long seq, hipStream_t s) { hipLaunchKernelGGL(k_wait_flag, dim3(1), dim3(64), 0, s, v, idx, seq); }
void launch_signal_flag(const DevView& v, int idx, hipStream_t s) { hipLaunchKernelGGL(k_signal_flag, dim3(1), dim3(64), 0, s, v, idx); }
void launch_reproj_res(const DevView& v, int state, double mult, hipStream_t s) {
  if (v.n_tiles == 0) return;
  hipLaunchKernelGGL(k_reproj_res, dim3(tiles_grid(v)), dim3(256), 0, s, v, state, mult);
}
void launch_reset_state(const DevView& v, const double* pose0, const double* cam0, const double* vel0, const double* imu0, hipStream_t s) {
  const int blocks = std::max(1, std::min(256, (v.n_frames * kPoseStride + 255) / 256));
  hipLaunchKernelGGL(k_reset_state, dim3(blocks), dim3(256), 0, s, v, pose0, cam0, vel0, imu0);
}
void launch_sum_tile_cost(const DevView& v, double* out, hipStream_t s) {
  hipLaunchKernelGGL(k_sum_tiles, dim3(1), dim3(256), 0, s, v, out);
}
void launch_cam_sq(const DevView& v, double* out, hipStream_t s) {
  hipLaunchKernelGGL(k_cam_sq, dim3(v.n_cams), dim3(256), 0, s, v, out);
}
void launch_outlier_mask(const DevView& v, int state, const double* thresh, unsigned char* mask, hipStream_t s) {
  if (v.n_tiles == 0) return;
  hipLaunchKernelGGL(k_outlier_mask, dim3(tiles_grid(v)), dim3(256), 0, s, v, state, thresh, mask);
}

}  // namespace vc
